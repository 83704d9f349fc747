/*
 * scatten.h — C ABI of libscatten_hip.so, the MI355X (gfx950) implementation of the
 * SCAttenNet spatial-coordinate-attention hot path.
 *
 * Every entry point takes plain device pointers, sizes and a hipStream_t (passed as
 * void*), never allocates, never synchronises, and is safe under hipGraph stream capture.
 * Each returns 0 on success or a nonzero SCA_ERR_* code (the Python layer maps it to an
 * exception; sca_last_error() gives the message).  All floating point is fp32.
 *
 * Reference interfaces replaced (tinh2044/SCAttenNet @ 2025-07-18; the reference is pure
 * PyTorch, so each entry point replaces an ATen op sequence, not a reference kernel):
 *   sca_gemm               nn.Linear forward/backward in model/attention.py:23-26,41-44,
 *                          49-51,74,101-103,126 ; model/layers.py:97-99,106-108 ;
 *                          model/fusion.py:31-34 ; model/residual.py:14-19
 *                          (q-scaling after bias :49, v-from-kv/2 :103, GELU :98 fused)
 *   sca_attn_fwd           attention.py:63-72 (SelfAttention), :115-124 (CrossAttention),
 *                          :165-178 (SelfCausalAttention) incl. model/utils.py:3-28 masks
 *   sca_attn_bwd           autograd of the same three op sequences
 *   sca_layernorm_fwd/bwd  nn.LayerNorm + the residual add in keypoint_module.py:67-72,
 *                          :101-111 and the position embedding add layers.py:15-30
 *   sca_reduce_rows        bias / LayerNorm-affine / position-table gradient reductions
 *   sca_coord_map_fwd/bwd  KeypointModule stream slicing + CoordinateMapping
 *                          (model/__init__.py:133-142, keypoint_module.py:22-26,
 *                          layers.py:111-123)
 *   sca_maxpool_t_fwd/bwd  ResidualBlock MaxPool1d(2,2) over frames (residual.py:40-43)
 *   sca_softmax_rows_*     CoordinatesFusion softmax (fusion.py:52-53)
 *   sca_gelu_bwd           GELU backward where no GEMM epilogue can absorb it
 *                          (fusion.py:43-50,74-77)
 *   sca_dropout            F.dropout in training mode (keypoint_module.py:64,100,164-165,
 *                          layers.py:105,107, fusion.py:48,54) with a counter-based mask;
 *                          also fused into the GEMM and LayerNorm epilogues
 *   sca_ctc_loss_fwd/bwd   MSCA_Net.compute_loss (model/__init__.py:241-290): log_softmax,
 *                          clamp(-100, 0), nn.CTCLoss(blank=0, reduction='none',
 *                          zero_infinity=True), finite mean, clamp(0, 100)
 *   sca_seqkd_fwd/bwd      SeqKD (loss.py:5-21) with the distillation weight and
 *                          clamp(-100, 100) of model/__init__.py:203-214
 *   sca_clamp              RecognitionHead logit clamp(+-50) (model/__init__.py:54-58)
 *   sca_lstm_cell_fwd/bwd  AlignmentModule's bidirectional nn.LSTM cell
 *                          (model/alignment_module.py:24-30, :68-69)
 *   sca_*_valid_fwd/bwd    the softmax, SeqKD and LSTM cell above restricted to a device-side
 *                          valid-frame count (batches padded to a length bucket)
 *   sca_optim_grad_sqnorm  torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
 *   sca_optim_scale_grads  (opt.py:34) and the NaN-loss test of opt.py:32
 *   sca_optim_adam_step    optimizer.step() (opt.py:35) of the torch.optim.Adam built by
 *                          optimizer.py:49-66, one parameter group per model child
 *   sca_ctc_greedy_decode  utils.ctc_decode (utils.py:164-189: tf.nn.ctc_beam_search_decoder
 *   sca_ctc_beam_decode    on the host) as evaluate_fn calls it (opt.py:84-89)
 *   sca_wer_counts         metrics.wer_single / edit_distance / get_alignment
 *                          (metrics.py:2793-2907)
 *   sca_ctc_*_decode_heads the decode loop of evaluate_fn over every evaluated head of one
 *                          forward (opt.py:76-89), one grouped call
 *   sca_eval_accumulate    wer_single per (head, clip), the totals wer_list needs, the loss
 *                          meters' sums and the hypothesis log of evaluate_fn (opt.py:77-119),
 *                          kept in device memory across the steps of a pass
 *   sca_ctc_align_heads    (no counterpart: the reference has no forced alignment) gloss spans
 *   sca_eval_log_alignments  and confidences of given label sequences, and their log in a pass
 *   sca_ensemble_log_probs (no counterpart) the weighted mean of the heads' posteriors as
 *                          log-probabilities, decoded as one more head
 *   sca_ensemble_log_probs_bwd  (no counterpart) its vector-Jacobian product, which makes the
 *                          ensemble a tensor the training losses can be taken on
 *   sca_ensemble_log_probs_dw, _dw_bwd  (no counterpart) the same pair with learned weights, the
 *                          softmax of scores on the device, and the gradient of those scores
 *   sca_distill_heads_fwd/bwd  the SeqKD terms of model/__init__.py:203-214 for all students in one
 *                          call, with (no counterpart) the ensemble of G heads as the teacher,
 *                          formed on the fly
 *   sca_ctc_beam_decode*_nbest  (no counterpart; the interface of the decoder's top_paths) the N
 *   sca_nbest_rescore/mbr/gather  best labellings of the beam search, their rescoring with a
 *                          bigram gloss model, the posterior over the list and MBR selection
 *   sca_mwer_fwd/bwd, sca_mwer_heads_fwd/bwd  (no counterpart) the minimum-WER training loss over
 *                          an n-best list: one head, or G heads with the reference as one more
 *                          entry and the gloss model's prior inside the posterior
 *   sca_finite_scan      the isnan().any() / isinf().any() tests of MSCA_Net.forward
 *                          (model/__init__.py:130-235), all tensors in one launch
 *   sca_step_report        total_loss (model/__init__.py:207,237), the loss terms the
 *                          training loop logs (opt.py:39-42) and the device-side form of
 *                          the non-finite skip (opt.py:32) over every checked tensor
 */
#ifndef SCATTEN_H
#define SCATTEN_H

#ifdef __cplusplus
extern "C" {
#endif

#define SCA_OK 0
#define SCA_ERR_ARG 1      /* invalid shape / alignment / argument */
#define SCA_ERR_LAUNCH 2   /* hipLaunchKernel failed */

#define SCA_GEMM_MAX_PROBLEMS 16
#define SCA_GEMM_MAX_SEGS 3

/* GEMM layouts: C[M,N] = sum_seg alpha_s * op(A_s) op(B_s)                           */
#define SCA_GEMM_NT 0  /* A[M,K] row-major, B[N,K] row-major  (Linear forward)          */
#define SCA_GEMM_NN 1  /* A[M,K] row-major, B[K,N] row-major  (Linear dX = dY W)        */
#define SCA_GEMM_TN 2  /* A[K,M] row-major, B[K,N] row-major  (Linear dW = dY^T X)      */

/* Epilogue flags (applied in this order):
 *   v = acc ; v += bias[n] ; v *= post_scale ;
 *   GELU : aux_out[m,n] = v ; v = gelu_erf(v)
 *   DROPOUT: v *= keep(drop_seed, m*N + n) / (1 - drop_p)   (see sca_dropout)
 *   DGELU: v *= gelu_erf'(aux[m,n])
 *   v += resid[m,n] (if resid) ; ACCUM: v += C[m,n] ; C[m,n] = v
 * so the post-LN blocks' y = x + dropout(Linear(h)) (keypoint_module.py:64,100 and
 * layers.py:105,107) is one epilogue, and the backward of dropout(GELU(z)) is DROPOUT|DGELU
 * with the forward's seed.                                                             */
#define SCA_EPI_GELU 1
#define SCA_EPI_DGELU 2
#define SCA_EPI_ACCUM 4
#define SCA_EPI_DROPOUT 8

typedef struct {
  const float* A;
  const float* B;
  int lda, ldb;
  int K;       /* reduction length of this segment (any: K, lda, ldb not multiples of 4 or
                  operands not 16-byte aligned take the element-wise load form) */
  float alpha; /* scales A on load: alpha=0.5 reproduces v_proj(kv/2) exactly */
} sca_gemm_seg;

typedef struct {
  sca_gemm_seg seg[SCA_GEMM_MAX_SEGS];
  int nseg;
  int M, N;
  float* C;
  int ldc;
  int epi;
  const float* bias; /* [N] or NULL */
  float post_scale;
  const float* resid; /* [M, ldr] or NULL */
  int ldr;
  const float* aux; /* DGELU input [M, ldx] */
  int ldx;
  float* aux_out; /* GELU pre-activation output [M, ldo] */
  int ldo;
  /* TN layout only: bias_grad[m] = bias_grad_scale * sum_k alpha*A[k, m] (the Linear bias
   * gradient colsum(dY), fused into the weight-gradient GEMM), or NULL */
  float* bias_grad;
  float bias_grad_scale;
  unsigned long long drop_seed; /* DROPOUT: per-call seed (one mask per seed) */
  float drop_p;                 /* DROPOUT: drop probability in [0, 1) */
} sca_gemm_problem;

/* Grouped GEMM over `nprob` independent problems (e.g. q/k/v x streams).
 * splitk > 1 (single segment per problem; shapes may differ) writes fp32 partial slabs
 * into `workspace` (splitk * sum_p (M_p * N_p + M_p) floats) and reduces them in a second
 * launch in fixed order (deterministic).                                                  */
int sca_gemm(int layout, int nprob, const sca_gemm_problem* probs, int splitk, float* workspace,
             void* stream);
/* The two launches of a split-K sca_gemm issued separately (same arguments): the GEMM
 * writing the slabs, then the fixed-order reduction + epilogue (lets a caller time them
 * apart, or put work between them).  sca_gemm_partial with splitk == 1 is sca_gemm.     */
int sca_gemm_partial(int layout, int nprob, const sca_gemm_problem* probs, int splitk, float* workspace,
                     void* stream);
int sca_gemm_reduce(int layout, int nprob, const sca_gemm_problem* probs, int splitk, float* workspace,
                    void* stream);
/* Split-K with the slab combine inside the GEMM launch (no second launch): every split writes
 * its partial slab write-through and takes a ticket on its output tile's counter; the last
 * arriver sums the slabs in slice order (deterministic) and runs the epilogue.
 * `counters`: sca_gemm_splitk_counters(nprob, max M, max N) unsigned ints, ZERO on entry and
 * left zero on exit (the last arriver resets its tile's counter), so one zeroed buffer serves
 * any number of launches that do not run concurrently on the same counters.  Falls back to
 * the two-launch form when the LDS-DMA kernel cannot take the shapes.                      */
long sca_gemm_splitk_counters(int nprob, int maxM, int maxN);
int sca_gemm_splitk_fused(int layout, int nprob, const sca_gemm_problem* probs, int splitk, float* workspace,
                          unsigned* counters, void* stream);

/* NT GEMM + post-LN LayerNorm in one launch (d_model = 256): per problem
 *   C = resid + dropout((A B^T + bias) * post_scale)      (exactly sca_gemm's NT epilogue)
 *   y = (C - mean) * rstd * gamma + beta,  rstd = 1 / sqrt(var + eps)   (nn.LayerNorm)
 * over each full row of C; mean / rstd saved per row (as sca_layernorm_fwd).  Replaces the
 * out-projection / fc2 GEMM + LayerNorm pairs of keypoint_module.py:63-72, 99-109.
 * Requires nseg == 1, N == 256, K a positive multiple of 32, 16-byte aligned operands with
 * leading dimensions multiple of 4 (y has leading dimension 256), epi 0 or DROPOUT only;
 * else SCA_ERR_ARG (use sca_gemm + sca_layernorm_fwd).                                    */
/* Optional chained NT GEMMs on the LayerNorm output y (same launch, the 32-row tile): pass p
 * computes C_p = epi((y B_p^T + bias_p) * post_scale_p) for one 256-row block B_p of an
 * nn.Linear weight ([256, 256] k-contiguous, row stride ldb), epi 0 or SCA_EPI_GELU (then
 * aux_out receives the pre-activation) — the next op's projection (an FFN's fc1 = 3 passes,
 * an attention block's q / k / v = 3 passes) without re-reading y or a launch boundary.    */
typedef struct {
  const float* B;
  int ldb;
  const float* bias; /* [256] or NULL */
  float post_scale;
  int epi;
  float* C;
  int ldc;
  float* aux_out;
  int ldo;
} sca_gemm_chain_pass;

typedef struct {
  const float* gamma; /* [N] */
  const float* beta;  /* [N] */
  float* y;           /* [M, N] */
  float* mean;        /* [M] */
  float* rstd;        /* [M] */
  int npass;          /* 0..3 chained passes */
  sca_gemm_chain_pass pass[3];
} sca_gemm_ln_problem;
#define SCA_GEMM_LN_MAX_PROBLEMS 8

int sca_gemm_ln(int nprob, const sca_gemm_problem* probs, const sca_gemm_ln_problem* ln, float eps,
                void* stream);
/* Row-tile height (32 or 16) sca_gemm_ln launches for nprob problems of at most maxM rows,
 * chained passes or not — the rule the launcher applies (SCA_GEMM_LN_BM overrides without
 * chained passes); hosts use it to name the kernel variant in their profiles. */
int sca_gemm_ln_rows(int nprob, int maxM, int chain);
/* Force the unchained tile height: bm = 16 or 32, 0 = the rule above (process-global;
 * SCA_GEMM_LN_BM sets the initial value, read once). */
int sca_gemm_ln_force_rows(int bm);

/* NN input-gradient GEMM + the backward of the LayerNorm that produced its input, in one
 * launch (d_model = 256).  Per problem:
 *   C  = resid + sum_s alpha * A_s B_s           (sca_gemm NN, epilogue: resid only)
 *      = dL/dy, the gradient w.r.t. the output y of an nn.LayerNorm whose input was x
 *   dx = rstd * (C*gamma - mean_n(C*gamma) - xhat * mean_n(C*gamma*xhat)),
 *        xhat = (x - mean) * rstd                  (aten native_layer_norm_backward)
 *   partial[0][blk][n] = sum_{rows of blk} C * xhat,  partial[1][blk][n] = sum C
 *        (fixed-order dgamma / dbeta partials per 32-row block; blk = row / 32, reduce
 *        them with sca_reduce_rows over nblk = sca_gemm_lnb_blocks(M) rows)
 * Replaces the input-gradient GEMM of a post-LN block's first op (the attention block's
 * dX = dq Wq + dk Wk + dv Wv + dY, the FFN's dx = dz W1 + dY) followed by the separate
 * LayerNorm backward of the block below (keypoint_module.py:69-72, 105-109), and, with
 * `wo`, that block's out-projection input-gradient GEMM as well.
 * Requires N == 256, 1..3 segments with K a positive multiple of 32 and one alpha, B
 * k-major (B[k][n] at B + k*ldb + n), 16-byte aligned operands, leading dimensions
 * multiples of 4; else SCA_ERR_ARG.                                                       */
typedef struct {
  const float* x;     /* [M, 256] LayerNorm input saved by the forward */
  const float* mean;  /* [M] */
  const float* rstd;  /* [M] */
  const float* gamma; /* [256] */
  float* dx;          /* [M, 256] gradient w.r.t. x */
  float* partial;     /* [2, nblk, 256] dgamma / dbeta partials */
  /* optional chained GEMM (NULL = none): dout = dx Wo, Wo [256, 256 * npass] row-major
   * (an nn.Linear weight [out, in]: dout is the gradient of the Linear's INPUT when dx is the
   * gradient of its output), in the same launch — the out-projection input gradient of the
   * attention block that produced the LayerNorm input (attention.py:74 backwards, npass 1),
   * or the FFN's dz = (dx W2) * gelu'(aux) (layers.py:104-107 backwards, npass 3, aux = the
   * fc1 pre-activation)                                                                     */
  const float* wo;
  float* dout;        /* [M, 256 * npass] */
  const float* aux;   /* NULL, or [M, 256 * npass]: dout *= gelu'(aux) (exact-erf GELU) */
  int npass;          /* 1..3 (0 reads as 1) */
  int ldw;            /* row stride of wo, dout and aux (0 reads as 256 * npass) */
  /* optional position table (NULL = none): the LayerNorm input is x + tab[(row % tab_T) + 2]
   * — the embedding LayerNorm of keypoint_module.py:154-160 (x = the mapped coordinates,
   * tab = LearningPositionEmbedding.weight [>= tab_T + 2, 256], layers.py:15-30)          */
  const float* tab;
  int tab_T;
} sca_gemm_lnb_problem;

int sca_gemm_lnb(int nprob, const sca_gemm_problem* probs, const sca_gemm_lnb_problem* lnb, void* stream);
int sca_gemm_lnb_blocks(int M);

/* Tuning knob: force the kernel variant of one layout for every later sca_gemm* call
 * (0 = built-in heuristic; 1 / 5 / 7 register-staged 64x64 / single-buffered 64x64 /
 * 128x64 8 waves; 20 / 21 / 22 LDS-DMA 64x64 with a 3- / 2- / 4-stage ring; TN only: 36 / 37
 * the k-split weight-gradient kernel with a 3- / 4-stage ring, 46 the same with the
 * register-staged interleaved operand stream, 38 / 39 / 40 / 43 128x128 register-staged
 * (43: interleaved phases); NT / NN only: 41 / 42 / 44 128x128 and 45 64x64 register-staged
 * (44, 45: interleaved) — every variant computes the full result; a shape a variant cannot
 * take runs on the LDS-DMA kernels).  Any other id: SCA_ERR_ARG, nothing changed.
 * Process-global.                                                                          */
int sca_gemm_tile_override(int layout, int tile);
/* sca_gemm with the kernel variant chosen for this call only (ids as above, 0 = the override
 * or heuristic; an invalid id is SCA_ERR_ARG): split-K slabs combined in-launch when
 * `counters` is given and the variant can (sca_gemm_splitk_fused), else the two-launch form. */
int sca_gemm_variant(int layout, int nprob, const sca_gemm_problem* probs, int splitk, float* workspace,
                     unsigned* counters, int variant, void* stream);

/* The kernel a sca_gemm_variant launch of these problems would run (variant 0: the override or
 * the heuristic), as a short name ("gemm_tnk_kernel<3, 1, true>", ...) written into buf
 * (NUL-terminated, truncated to len).  Host-only: no GPU call; for profiling records.      */
int sca_gemm_kernel_name(int layout, int nprob, const sca_gemm_problem* probs, int splitk, int variant, char* buf,
                         int len);

/* Fused masked attention over (B, T, H*hd) row-major activations (head h at columns
 * h*hd .. h*hd+hd-1, row stride ld*).  Scores use q as given (the projection already
 * applied hd^-0.5).  Masking, per query row i and key j:
 *   causal && j > i                    -> -inf            (attention.py:165-169)
 *   add_mask != NULL                   -> s + add_mask[b, (h,) i, j]   (general (B,1|H,Tq,Tk))
 *   else key_valid != NULL && !valid_j -> finfo.min       (utils.py:3-12)
 *   else                               -> s + (causal && plus_one ? 1 : 0) (utils.py:24-27)
 * Softmax stats are saved per (g,b,h,i) in the base-2 domain the kernels compute in
 * (scores x log2(e)): m (row max) and ll (log2 of the row sum), kept apart so that fully
 * padded rows (all finfo.min) recompute to exactly uniform weights.  A materialised mask
 * value so negative that x log2(e) overflows is taken as finfo.min (it only arises from
 * finfo.min masks, whose sums with a score all round to finfo.min).                    */
typedef struct {
  const float* q;
  const float* k;
  const float* v;
  float* o;
  float* stat_m;  /* [B*H*Tq] */
  float* stat_ll; /* [B*H*Tq] */
  const float* key_valid; /* [B, Tk] 1.0/0.0, or NULL */
  const float* add_mask;  /* [B, Tq, Tk] additive, or NULL */
  /* attention-probability dropout (attention.py:67-69, 119-121, 173-175), drop_p = 0: none.
   * O = (P * keep / (1 - drop_p)) V with keep = the sca_dropout mask of drop_seed over the
   * (B, H, Tq, Tk) probabilities, element e = ((b H + h) Tq + i) Tk + j (mod 2^32); the
   * softmax statistics are those of P.  The backward must get the same seed and p.        */
  unsigned long long drop_seed;
  float drop_p;
  /* add_mask layout: 0 or 1 = [B, Tq, Tk] shared by every head; H = [B, H, Tq, Tk], one mask
   * per head (the reference adds any mask broadcastable to (B, H, Tq, Tk), attention.py:65) */
  int mask_heads;
} sca_attn_fwd_problem;

typedef struct {
  const float* q;
  const float* k;
  const float* v;
  const float* o;
  const float* dout;
  const float* stat_m;
  const float* stat_ll;
  const float* key_valid;
  const float* add_mask;
  float* dq;    /* written (not accumulated), scaled by dq_scale */
  float* dk;
  float* dv;
  float* delta; /* workspace [B*H*Tq] : rowsum(dO * O) */
  float dq_scale;
  float dv_scale;
  float* dq_part; /* workspace of sca_attn_bwd_workspace() floats, or NULL: with it (hd 32, no
                     add_mask) the backward is one fused launch over 256-key blocks + a
                     fixed-order dQ reduction; without it the split dq / dkdv kernels */
  unsigned long long drop_seed; /* the forward's attention-probability dropout */
  float drop_p;
  int mask_heads;               /* as sca_attn_fwd_problem */
} sca_attn_bwd_problem;

#define SCA_ATTN_MAX_PROBLEMS 8

int sca_attn_fwd(int nprob, const sca_attn_fwd_problem* probs, int B, int H, int Tq, int Tk, int hd,
                 int ldq, int ldk, int ldv, int ldo, int causal, int plus_one, void* stream);
/* dq_part floats per problem for the fused hd-32 backward (0 when that path does not apply) */
long sca_attn_bwd_workspace(int B, int H, int Tq, int Tk, int hd);
int sca_attn_bwd(int nprob, const sca_attn_bwd_problem* probs, int B, int H, int Tq, int Tk, int hd,
                 int ldq, int ldk, int ldv, int ldo, int causal, int plus_one, void* stream);
/* Backward kernel choice: enable = 1 (default) runs the single-launch fused kernel where it
 * applies (hd 16, Tq and Tk <= 256, no add_mask): S / P / dP / dS once per score, dK / dV in
 * registers, dQ from an LDS image of dS; enable = 0 always runs the split dq + dkdv pair.
 * Both are deterministic and write dq, dk, dv and delta.                               */
int sca_attn_bwd_fused(int enable);

/* y = act(LayerNorm(x + r) * gamma + beta + post) over rows of width N (eps given).
 * r row index = (row % r_mod) + r_off  (r_mod = rows for an ordinary residual; r_mod = T,
 * r_off = 2 for the LearningPositionEmbedding table); post (or NULL) is row-aligned with x;
 * act: 0 = identity, 1 = ReLU (ResidualBlock, model/residual.py:31-38).
 * drop_p > 0 (act must be identity): y = dropout(y) with the sca_dropout mask of
 * drop_seed — the embedding dropout after first_*_norm (keypoint_module.py:164-165); the
 * backward applies the same mask to dy (sca_dropout) before sca_layernorm_bwd.
 * Saves mean/rstd per row.  Any N (widths over 1024 take a row-looping kernel).         */
#define SCA_ACT_NONE 0
#define SCA_ACT_RELU 1
typedef struct {
  const float* x;
  const float* r; /* or NULL */
  const float* gamma;
  const float* beta;
  const float* post; /* or NULL */
  float* y;
  float* mean;
  float* rstd;
  int act;
  unsigned long long drop_seed;
  float drop_p;
} sca_ln_fwd_problem;

typedef struct {
  const float* dy;
  const float* x;
  const float* r;
  const float* gamma;
  const float* mean;
  const float* rstd;
  const float* y;  /* forward output, read when act == ReLU (gradient gate y > 0) */
  int act;
  float* dpost;  /* or NULL: receives the (gated) gradient of `post` */
  float* dx;     /* gradient of (x + r); ACCUM adds into dx */
  float* dgamma; /* [N] written; NULL: the affine partials stay in `partial` (rows 0..nblk-1
                  * sum to dgamma, rows nblk..2nblk-1 to dbeta) for a later sca_reduce_rows */
  float* dbeta;  /* [N] written (ignored when dgamma is NULL) */
  float* partial; /* workspace [2 * nblk * N], nblk from sca_layernorm_bwd_blocks() */
} sca_ln_bwd_problem;

#define SCA_LN_MAX_PROBLEMS 8
int sca_layernorm_fwd(int nprob, const sca_ln_fwd_problem* probs, int rows, int N, int r_mod, int r_off,
                      float eps, void* stream);
int sca_layernorm_bwd_blocks(int rows);
int sca_layernorm_bwd(int nprob, const sca_ln_bwd_problem* probs, int rows, int N, int r_mod, int r_off,
                      int accumulate, void* stream);

/* MaxPool1d(kernel 2, stride 2) over the frame axis of (B, T, C) -> (B, T/2, C)
 * (ResidualBlock downsample, model/residual.py:40-43).  Backward routes each gradient to
 * the first maximal element of its pair (ties -> the earlier frame), like ATen.          */
typedef struct {
  const float* x;
  float* y;  /* forward */
  const float* dy;
  float* dx; /* backward (fully written, odd trailing frame gets 0) */
} sca_pool_problem;
#define SCA_POOL_MAX_PROBLEMS 8
int sca_maxpool_t_fwd(int nprob, const sca_pool_problem* probs, int B, int T, int C, void* stream);
int sca_maxpool_t_bwd(int nprob, const sca_pool_problem* probs, int B, int T, int C, void* stream);

/* Row softmax over the last dim (any N) and its backward (CoordinatesFusion's
 * unscaled, unmasked attention weights, model/fusion.py:52-53):
 *   fwd: y = softmax(x)            bwd: dx = y * (dy - sum_j dy_j y_j)                  */
typedef struct {
  const float* x;  /* fwd input */
  const float* y;  /* fwd output / bwd input */
  const float* dy;
  float* out;      /* fwd: y ; bwd: dx */
} sca_softmax_problem;
#define SCA_SOFTMAX_MAX_PROBLEMS 8
int sca_softmax_rows_fwd(int nprob, const sca_softmax_problem* probs, int rows, int N, void* stream);
int sca_softmax_rows_bwd(int nprob, const sca_softmax_problem* probs, int rows, int N, void* stream);

/* ---- valid-frame variants (length-bucketed batches) ----
 * A batch padded beyond its own longest clip to a fixed bucket length must not let the extra
 * frames reach the valid ones.  Three ops would (this softmax, SeqKD, the LSTM's reverse
 * direction); their *_valid entry points take
 *   valid_frames  device pointer to ONE int32: the batch's unpooled longest length,
 *   shift         the number of MaxPool1d(2, 2) stages in front of the op,
 * and use nv = clamp(*valid_frames >> shift, 1, T) as the valid length at the op (floor-halving
 * k times is >> k).  The scalar is read on the device: no host read, no allocation, and a
 * graph replay sees whatever the host last copied there.  With nv == T each variant computes
 * bitwise what its plain entry point does.
 *
 * sca_softmax_rows_valid_fwd: softmax over columns [0, nv) of every row; columns [nv, N) are
 * written as exact 0.  Its backward is sca_softmax_rows_bwd unchanged: y = 0 gives
 * dx = y * (dy - sum) = 0 there, and the row sum only collects the valid columns.          */
int sca_softmax_rows_valid_fwd(int nprob, const sca_softmax_problem* probs, int rows, int N,
                               const int* valid_frames, int shift, void* stream);

/* Elementwise GELU backward: dz = dy * gelu_erf'(z) over n elements (the pre-activation z
 * is what the GEMM GELU epilogue stored).                                               */
typedef struct {
  const float* dy;
  const float* z;
  float* dz;
} sca_gelu_bwd_problem;
#define SCA_GELU_MAX_PROBLEMS 8
int sca_gelu_bwd(int nprob, const sca_gelu_bwd_problem* probs, long n, void* stream);

/* Fixed-order sum of up to SCA_SUM_MAX_TERMS same-shaped tensors, n elements each:
 * out = in[0] + in[1] + ... + in[nin-1] (left to right) — the gradient of a tensor read by
 * several ops (the final x-stream map read by every merge layer, keypoint_module.py:181-187)
 * in one launch per group instead of one autograd add per pair.  16-byte aligned.         */
#define SCA_SUM_MAX_TERMS 8
typedef struct {
  const float* in[SCA_SUM_MAX_TERMS];
  int nin;
  float* out;
} sca_sum_problem;
#define SCA_SUM_MAX_PROBLEMS 8
int sca_sum_tensors(int nprob, const sca_sum_problem* probs, long n, void* stream);

/* Dropout (F.dropout, training mode) over contiguous (rows, cols) tensors:
 *   y[e] = x[e] * keep(seed, e) / (1 - p),  e = row * cols + col
 * keep() is a counter-based hash RNG (no state, no sequence): with
 *   mix(x) = lowbias32 (x^=x>>16; x*=0x7feb352d; x^=x>>15; x*=0x846ca68b; x^=x>>16),
 *   key = mix(lo32(seed) ^ mix(hi32(seed) + 0x9e3779b9)),
 *   keep = mix(mix(e ^ key) + key) >= (uint32)(p * 2^32 in fp32)
 * so forward, backward and the CPU oracle regenerate the same mask from the seed alone
 * (masks differ from torch's Philox stream; the drop rate is the same).  The same mask
 * is applied by the GEMM DROPOUT epilogue and the LayerNorm forward.  In-place allowed.
 * Used for: the backward of every dropout site, and the fusion's attention-weight and
 * output dropout (model/fusion.py:48,54).                                               */
typedef struct {
  const float* x;
  float* y;
  unsigned long long seed;
} sca_dropout_problem;
#define SCA_DROPOUT_MAX_PROBLEMS 12
int sca_dropout(int nprob, const sca_dropout_problem* probs, long rows, int cols, float p, void* stream);

/* Key validity of the (B, T) attention mask the SCA stack receives, as the (B, T) fp32 1/0
 * vector the attention kernels read (key_valid):
 *   key_valid[i] = ((float)mask[i] == 1.0f) ? 1 : 0
 * — the reference's predicate: create_attention_mask / create_causal_attention_mask
 * (model/utils.py:8-12, 19-23) cast the mask to fp32 and mask every key where
 * 1.0 - mask != 0, so only the value 1 keeps a key (2, 0.5, -1, NaN all mask it).
 * dtype: the mask's element type (SCA_MASK_*); any alignment; n = 0 is a no-op.        */
#define SCA_MASK_F32 0
#define SCA_MASK_F64 1
#define SCA_MASK_I64 2
#define SCA_MASK_I32 3
#define SCA_MASK_U8 4   /* bool / uint8 */
#define SCA_MASK_F16 5
#define SCA_MASK_BF16 6
#define SCA_MASK_I8 7
#define SCA_MASK_I16 8
int sca_key_valid(const void* mask, int dtype, float* key_valid, long n, void* stream);

/* p[0 .. n) = 0 (fp32): the gradient buffers a backward only partly writes (the position
 * table's rows that no frame reads, model/layers.py LearningPositionEmbedding) — one launch
 * in the captured step instead of an ATen fill.                                          */
int sca_zero(float* p, long n, void* stream);

/* Registers a device-resident step counter (or NULL) read by every dropout mask at run
 * time: effective seed = seed + counter * 0x9E3779B97F4A7C15.  A hipGraph that captures
 * the counter's increment then draws fresh masks on every replay although the seeds in
 * its kernel arguments are frozen.  Process-global; applies to launches issued after. */
int sca_dropout_offset(const unsigned long long* counter);

/* out[i, j] (+)= scale * sum_{s < S} in[s * stride_s + i * stride_i + j],  i < I, j < N.
 * Column sums (bias gradients), slab reductions, position-table gradients.            */
typedef struct {
  const float* in;
  float* out;
  float scale;
} sca_reduce_problem;

#define SCA_REDUCE_MAX_PROBLEMS 64
int sca_reduce_rows(int nprob, const sca_reduce_problem* probs, int S, int I, int N, long stride_s,
                    long stride_i, int accumulate, void* stream);

/* Coordinate mapping of one stream (fused A1+A2): keypoints (B*T, K_all, 2) fp32,
 * joint index list idx[K] (int32, device) ->
 *   xe[row, n] = sum_k kp[row, idx[k], 0] * Wx[n, k] + bx[n]
 *   ye[row, n] = sum_k kp[row, idx[k], 1] * Wy[n, k] + by[n]                           */
typedef struct {
  const float* kp;
  const int* idx;
  int K;
  const float* wx;
  const float* bx;
  const float* wy;
  const float* by;
  float* xe;
  float* ye;
} sca_coord_map_problem;

typedef struct {
  const float* kp;
  const int* idx;
  int K;
  const float* wx;
  const float* wy;
  const float* dxe;
  const float* dye;
  float* dwx;     /* [N, K] written */
  float* dwy;     /* [N, K] written */
  float* dkp;     /* [rows, K_all, 2] accumulated into (must be zeroed by caller) or NULL */
  float* partial; /* workspace [2 * nchunk * N * K], nchunk = sca_coord_map_bwd_chunks(rows) */
} sca_coord_map_bwd_problem;

#define SCA_MAP_MAX_PROBLEMS 8
int sca_coord_map_fwd(int nprob, const sca_coord_map_problem* probs, int rows, int K_all, int N,
                      void* stream);
int sca_coord_map_bwd_chunks(int rows);
int sca_coord_map_bwd(int nprob, const sca_coord_map_bwd_problem* probs, int rows, int K_all, int N,
                      void* stream);

/* Input contract: SLR_Dataset.normalize_keypoints
 * (dataset.py:134-170) on a zero-padded batch.  kp_in / kp_out: (B, T, K_all, 2) fp32;
 * frame t of clip b with t < lengths[b] is normalised part by part, in order (part p owns
 * joints part_idx[part_off[p] .. part_off[p+1])): its bounding box grown by 5 % of the
 * longer side and squared, clamped to [0, 1], then x, y mapped into it (an axis whose
 * clamped extent is 0 is left as is).  Frames t >= lengths[b] are written as zeros (the
 * collator's padding, dataset.py:82-91).  K_all <= 1024; kp_out may alias kp_in.        */
/* The sample pipeline of SLR_Dataset.data_collator for a batch in one launch
 * (dataset.py:58-125 with preprocess_keypoints :124-132): for t < lengths[b], frame (b, t)
 * is raw row src_row[b T + t] (frame selection, dataset.py:185-215, decided on the host with
 * the reference's RNG calls), transformed by the clip's augmentation affine (affine + 6 b =
 * [a00 a01 tx a10 a11 ty]: rotation about (0, 0) and / or x -> 1 - x, augmentation.py:3-25;
 * NULL = none) and then normalised as sca_normalize_parts (nparts = 0: not normalised);
 * frames t >= lengths[b] are zeros.  raw: (R, K_all, 2) fp32, all clips' frames.          */
int sca_prepare_keypoints(const float* raw, const int* src_row, const float* affine, const int* lengths,
                          float* kp_out, int B, int T, int K_all, const int* part_off, const int* part_idx,
                          int nparts, void* stream);
int sca_normalize_parts(const float* kp_in, float* kp_out, const int* lengths, int B, int T, int K_all,
                        const int* part_off, const int* part_idx, int nparts, void* stream);

/* ---- recognition-head losses --------------------------------
 * CTC over batch-major logits (B, T, C) (the reference's permute(1, 0, 2) at
 * model/__init__.py:245 is a view; no copy), labels (B, S) int32 padded, in_len / tgt_len
 * (B) int32 device vectors.  Per sample: S_b = max(tgt_len, 1), T_b = max(in_len, 1, S_b)
 * (model/__init__.py:262-266); the caller validates T_b <= T, S_b <= S and labels in [0, C)
 * (out-of-range values are clamped in-kernel only to stay in bounds).  nll (B, optional):
 * per-sample losses after zero_infinity; loss (1): clamp(mean over finite nll, 0, 100), 0
 * when none is finite.  ws: sca_ctc_workspace_floats(B, T, S) floats, kept between the
 * forward and the backward (row log-sum-exp, alpha, beta, per-sample gradient scale).
 * bwd: dlogits = d loss / d logits given dloss (1 float, device).  C <= 8192, S <= 1023. */
#define SCA_CTC_MAX_C 8192
#define SCA_CTC_MAX_S 1023
long sca_ctc_workspace_floats(int B, int T, int S);
int sca_ctc_loss_fwd(const float* logits, const int* labels, const int* in_len, const int* tgt_len, int B, int T,
                     int C, int S, float* nll, float* loss, float* ws, void* stream);
int sca_ctc_loss_bwd(const float* logits, const int* labels, const int* in_len, const int* tgt_len, int B, int T,
                     int C, int S, const float* dloss, const float* ws, float* dlogits, void* stream);

/* ---- evaluation: CTC decoding and WER counts (opt.py:50-128) ----------------------------
 * Decoders over the same batch-major fp32 logits (B, T, C); blank = class 0 (the reference's
 * column rotation and "+ 1", utils.py:168-183, cancel: ids are the model's class indices).
 * in_len (B) int32 device, clamped in-kernel to [0, T].  tokens (B, T) int32 padded with 0,
 * out_len (B) int32, score (B) fp32.  ws: sca_ctc_decode_workspace_bytes(B, T, C, W) bytes
 * (0 for unsupported sizes; the greedy decoder needs W = 1), 8-byte aligned.
 *
 * sca_ctc_greedy_decode: per frame the arg-max over C (ties to the lowest class), repeats
 * collapsed, blanks dropped; score = the sum of the arg-max log-probabilities.
 *
 * sca_ctc_beam_decode: CTC prefix beam search in log space, the algorithm of
 * tf.nn.ctc_beam_search_decoder (utils.py:172-177) with top_paths = 1 and no label merging
 * inside the search; 1 <= beam_width <= 32, C <= 8192.  A beam is a label prefix with
 * lb (ends in blank), ll (ends in its last label), total = logaddexp(lb, ll); start: the
 * empty prefix with lb = 0, ll = -inf.  Frame t < in_len[b], lp = log_softmax(logits[b, t]):
 *   every active beam p with last label e:  lb' = total + lp[0];  ll' = ll + lp[e] (-inf for
 *     the empty prefix);  if p's parent prefix q is an active beam, ll' = logaddexp(ll',
 *     lp[e] + (e == last(q) ? lb_q : total_q))
 *   every active beam q and label c != 0 whose prefix q + c is not an active beam is a
 *     candidate with lb = -inf, ll = lp[c] + (c == last(q) ? lb_q : total_q); candidates at
 *     -inf are dropped
 *   the new beams are the beam_width best of both sets by total; ties: updated beams before
 *     candidates, then the lower beam slot, then the lower class.
 * The result is the best beam by total after the last frame (ties to the lower slot); score
 * is its total; in_len = 0 gives the empty hypothesis with score 0.  collapse_repeats != 0
 * merges adjacent equal labels of the result (the groupby of utils.py:185-188, which
 * collapses genuine repeats too).                                                          */
#define SCA_CTC_MAX_BEAM 32
long sca_ctc_decode_workspace_bytes(int B, int T, int C, int W);
int sca_ctc_greedy_decode(const float* logits, const int* in_len, int B, int T, int C, int* tokens, int* out_len,
                          float* score, void* ws, void* stream);
int sca_ctc_beam_decode(const float* logits, const int* in_len, int B, int T, int C, int beam_width,
                        int collapse_repeats, int* tokens, int* out_len, float* score, void* ws, void* stream);

/* counts (N, 4) int32 = (num_del, num_ins, num_sub, num_ref) of metrics.wer_single
 * (metrics.py:2793-2907) per pair of ref (N, Rmax) / hyp (N, Hmax) int32 token rows, padded,
 * with lengths (N) int32 clamped in-kernel to [0, Rmax] / [0, Hmax]; Rmax, Hmax <= 128.
 * The matrix of metrics.edit_distance (del 3, ins 3, sub 4; equal tokens copy the diagonal
 * cell) and the back-trace of metrics.get_alignment (correct, substitution, insertion,
 * deletion, in this order of preference).  Cells are 16-bit: the wrap of the reference's
 * uint8 matrix once 3 (R + H) > 255 is not reproduced.                                     */
#define SCA_WER_MAX_LEN 128
int sca_wer_counts(const int* ref, const int* ref_len, const int* hyp, const int* hyp_len, int N, int Rmax,
                   int Hmax, int* counts, void* stream);

/* ---- evaluation step: grouped decoding and device-side totals (opt.py:50-128) -------------
 * The decoders above over G logit tensors at once, 1 <= G <= SCA_EVAL_MAX_HEADS: the heads of
 * one forward, all of shape (B, T, C), all decoded with the same in_len (B).  The G device
 * pointers travel by value in `heads` (as sca_finite_scan's tensors do: no device table,
 * nothing to upload, capturable).  tokens (G, B, T), out_len (G, B), score (G, B); ws:
 * sca_ctc_decode_heads_workspace_bytes(G, B, T, C, W) bytes (0 for unsupported sizes), 8-byte
 * aligned.  The row statistics and the per-frame best labels of all G B T rows are one launch
 * each, the frame recursion runs on a (B, G) grid, and every (head, clip) has its own arena
 * slice and cls / clp rows: head g's results are bitwise those of the single-head entry point
 * called on heads->logits[g].
 *
 * All eight decoders (these four, the n-best and the fused forms below) are one argument check
 * and one launcher; a single-head entry point is the grouped one with G = 1 and its tensor in
 * heads->logits[0].  The launcher enqueues the row statistics (the row pass of the CTC loss,
 * one body for both; with G = 1 the loss's own launch), the per-frame best labels for the beam
 * and n-best searches, and one search kernel; the three workspace-size functions are one formula, the single-head layout
 * over G B clips.                                                                          */
#define SCA_EVAL_MAX_HEADS 8
typedef struct {
  const float* logits[SCA_EVAL_MAX_HEADS]; /* entries [G, 8) are ignored */
} sca_decode_heads;
long sca_ctc_decode_heads_workspace_bytes(int G, int B, int T, int C, int W);
int sca_ctc_greedy_decode_heads(const sca_decode_heads* heads, int G, const int* in_len, int B, int T, int C,
                                int* tokens, int* out_len, float* score, void* ws, void* stream);
int sca_ctc_beam_decode_heads(const sca_decode_heads* heads, int G, const int* in_len, int B, int T, int C,
                              int beam_width, int collapse_repeats, int* tokens, int* out_len, float* score,
                              void* ws, void* stream);

/* ---- evaluation: n-best lists, bigram rescoring, MBR selection ------------------------------
 * sca_ctc_beam_decode_nbest / sca_ctc_beam_decode_heads_nbest: the N = nbest best labellings of
 * the search above, 1 <= nbest <= beam_width <= 32.  Logits, in_len, ws and its size are those
 * of sca_ctc_beam_decode / sca_ctc_beam_decode_heads (the one launcher's three launches; G = 1
 * for the single-head form).  tokens (G, B, N, T) int32 padded with 0, out_len (G, B, N) int32, score
 * (G, B, N) fp32, count (G, B) int32; every element is written by every call.
 *   The search is sca_ctc_beam_decode's, frame for frame.  After the last frame the active
 *   beams are in descending order of total, ties in slot order: entry n is beam n, its tokens
 *   the prefix walked back through the arena, its score offset + total_n (the arithmetic of the
 *   1-best score).  count = min(nbest, active beams); entries >= count have length 0, score
 *   -inf and tokens 0.  in_len = 0 gives count 1: the empty hypothesis with score 0.
 *   collapse_repeats = 0: nothing more is done, and entry 0 (tokens, length, score) is bitwise
 *   sca_ctc_beam_decode's result.
 *   collapse_repeats != 0: the groupby of utils.py:185-188 is applied to every entry.  Distinct
 *   prefixes can collapse to one labelling ((3) and (3, 3) both become (3)), and a list with
 *   the same hypothesis twice has no posterior, so entries that become equal are merged into
 *   the first of them, the survivor's score being the logaddexp of its own score and its
 *   duplicates' in ascending entry order (full-precision expf / log1pf).  The merged list is
 *   then re-sorted by score, descending; the sort is stable (ties to the lower entry); count is
 *   the merged count.  Entry 0 can therefore DIFFER from sca_ctc_beam_decode's collapsed
 *   result: two merged entries can overtake the best single beam (common with few classes,
 *   rare from some 20 classes on).
 * One lane per final beam walks and collapses its own prefix, each lane then looks for the
 * lowest earlier entry with equal labels, the survivors add up and a rank count re-sorts.  No
 * float atomics: deterministic, a replayed capture is bitwise the eager call, and head g's
 * rows are bitwise those of the single-head call on heads->logits[g].
 *
 * sca_nbest_rescore: the second pass over such a list.  lm: NULL, or a dense (C, C) fp32 table
 * of log-probabilities lm[prev * C + cur].  Class 0, the blank, is never a token and stands for
 * the sentence boundary: lm(h) = lm[0, h_0] + sum_i lm[h_{i-1}, h_i] + lm[h_{len-1}, 0], and
 * lm(empty) = lm[0, 0]; NULL means lm(h) = 0.  Tokens are clamped into [0, C) only to stay in
 * bounds.  For the valid entries n < count (count clamped to [0, N], lengths to [0, T]):
 *   total_n     = score_n + (lm_weight * lm(h_n) + length_bonus * len(h_n))
 *   posterior_n = softmax over the valid entries of posterior_scale * total_n
 *   order       = the valid entries by total descending, ties to the lower entry
 * Entries >= count have total -inf, posterior 0 and order[n] = n.  With lm_weight = 0 and
 * length_bonus = 0 (and finite lm values) total is score, bit for bit, and order the identity.
 * Specified for finite totals.  One wave per (head, clip); the len + 1 gathers of an entry are
 * independent and summed by a butterfly in a fixed order.  total, posterior (G, B, N) fp32,
 * order (G, B, N) int32.
 *
 * sca_nbest_mbr: minimum-Bayes-risk selection under the alignment of sca_wer_counts.
 *   loss (G, B, N, N) int32: loss[i, j] = num_del + num_ins + num_sub of wer_single with
 *     reference h_j and hypothesis h_i; 0 where i = j or an entry is not valid
 *   risk (G, B, N) fp32: risk_i = sum_j posterior_j * loss[i, j], j ascending; +inf for i >= count
 *   best (G, B) int32: the arg-min of risk, ties to the lower entry
 * T <= SCA_WER_MAX_LEN.  Two launches: one workgroup per ordered pair and (head, clip), then one
 * wave per (head, clip).
 *
 * sca_nbest_gather: entry sel[(g B + b) * sel_stride] (clamped to [0, N)) of every list as a
 * 1-best row: tokens1 (G, B, T) padded with 0, out_len1 (G, B), value1 (G, B) = value[.., entry]
 * (value (G, B, N) fp32: score or total).  sel = order with sel_stride = N selects by total,
 * sel = best with sel_stride = 1 selects by risk.  The aligner and sca_eval_accumulate take the
 * result as they take a decoder's.
 *
 * None of these allocates, copies or synchronises (capturable); arguments are validated before
 * any GPU call.                                                                              */
int sca_ctc_beam_decode_nbest(const float* logits, const int* in_len, int B, int T, int C, int beam_width, int nbest,
                              int collapse_repeats, int* tokens, int* out_len, float* score, int* count, void* ws,
                              void* stream);
int sca_ctc_beam_decode_heads_nbest(const sca_decode_heads* heads, int G, const int* in_len, int B, int T, int C,
                                    int beam_width, int nbest, int collapse_repeats, int* tokens, int* out_len,
                                    float* score, int* count, void* ws, void* stream);
int sca_nbest_rescore(const int* tokens, const int* out_len, const float* score, const int* count, int G, int B,
                      int N, int T, const float* lm, int C, float lm_weight, float length_bonus,
                      float posterior_scale, float* total, float* posterior, int* order, void* stream);
int sca_nbest_mbr(const int* tokens, const int* out_len, const int* count, const float* posterior, int G, int B,
                  int N, int T, int* loss, float* risk, int* best, void* stream);
int sca_nbest_gather(const int* tokens, const int* out_len, const float* value, const int* sel, int sel_stride,
                     int G, int B, int N, int T, int* tokens1, int* out_len1, float* value1, void* stream);

/* ---- evaluation: shallow fusion of the bigram gloss model into the beam search --------------
 * sca_ctc_beam_decode_fused_nbest / sca_ctc_beam_decode_heads_fused_nbest: the search of
 * sca_ctc_beam_decode_nbest with one change: what a beam is ranked by.  lm: NULL, or the dense
 * (C, C) fp32 table of sca_nbest_rescore (class 0 is the sentence boundary), C the logits'.
 * Every prefix p carries a bonus that depends on the prefix only:
 *   g(empty) = 0
 *   g(q + c) = g(q) + lm_weight * lm[last(q) (0 for the empty prefix), c] + length_bonus
 *   lb, ll, total, the update rule, the parent-merge rule and the candidate rule are unchanged
 *     and purely acoustic.  Two paths to the same prefix have the same g, so merging stays well
 *     defined, and a pruned prefix that comes back takes its arena node again.
 *   Per-frame cut: the beam_width best of updated beams and candidates by
 *     key = total + g(prefix); ties as in the unfused search: updated beams first, then the
 *     lower slot, then the lower class.
 *   After the last frame the beams are ordered by
 *     final key = total + g(p) + lm_weight * lm[last(p) (0 if empty), 0], ties to the lower slot:
 *     exactly the total sca_nbest_rescore computes for the uncollapsed entry with the same
 *     table, weight and bonus.  Entry n of the list is the n-th beam in that order.
 *   The outputs keep the n-best entry's format and meaning: score is the acoustic
 *     offset + total_n, not the key; tokens, out_len and count are as there.  With
 *     collapse_repeats the tail of sca_ctc_beam_decode_nbest (collapse, merge by logaddexp of the
 *     acoustic scores, stable re-sort by score) runs unchanged on that list.  sca_nbest_rescore,
 *     sca_nbest_mbr, sca_nbest_gather, the aligner and sca_eval_accumulate take the result as
 *     they take the unfused list's, and the rescorer with the same arguments turns the scores
 *     into the totals the search ranked by.
 *   lm = NULL means lm(.) = 0: the search is guided by the length bonus only.  With
 *     lm_weight = 0 and length_bonus = 0 every output is bitwise
 *     sca_ctc_beam_decode_heads_nbest's.  Specified for finite tables and finite weights of
 *     either sign; in_len = 0 gives count 1, the empty hypothesis, score 0.
 * A beam's candidates come from the W + 1 labels with the largest lp[c] + lm_weight * lm[last, c]
 * (ties to the lower class), selected per beam and frame over the whole row: the frame's shared
 * top-(W + 1) by lp is not exact once the order depends on the beam's last label.  At least W of
 * those labels differ from the beam's last label, and each of them has an item in the pool that
 * is no worse than any label left out, so the cut is the cut over all C - 1 labels.
 * g is carried relative to the best beam's, as the totals are.  Limits: those of the beam
 * decoder (1 <= nbest <= beam_width <= 32, C <= 8192).  ws: sca_ctc_fused_workspace_bytes(G, B,
 * T, C, W) bytes (0 for unsupported sizes; G = 1 for the single-head form), 8-byte aligned.  Two
 * launches (row statistics, frame recursion); no float atomics, deterministic, a replayed
 * capture is bitwise the eager call and head g of a grouped call is bitwise the single-head
 * call; nothing allocates, copies or synchronises, and arguments are validated before any GPU
 * call.                                                                                      */
long sca_ctc_fused_workspace_bytes(int G, int B, int T, int C, int W);
int sca_ctc_beam_decode_fused_nbest(const float* logits, const int* in_len, int B, int T, int C, int beam_width,
                                    int nbest, int collapse_repeats, const float* lm, float lm_weight,
                                    float length_bonus, int* tokens, int* out_len, float* score, int* count,
                                    void* ws, void* stream);
int sca_ctc_beam_decode_heads_fused_nbest(const sca_decode_heads* heads, int G, const int* in_len, int B, int T,
                                          int C, int beam_width, int nbest, int collapse_repeats, const float* lm,
                                          float lm_weight, float length_bonus, int* tokens, int* out_len,
                                          float* score, int* count, void* ws, void* stream);

/* ---- training: minimum word error rate (MWER) loss over an n-best list ----------------------
 * The expected number of errors of a clip's n-best hypotheses under the model's own posterior
 * over that list, with exact CTC likelihoods, and its gradient with respect to the logits.
 * Inputs: batch-major fp32 logits (B, T, C), blank = class 0; in_len (B) clamped to [0, T] as
 * the decoders clamp it; a list in sca_ctc_beam_decode_nbest's format, tokens (B, N, H) int32,
 * out_len (B, N) clamped to [0, H], count (B) clamped to [0, N]; references ref (B, R) int32,
 * ref_len (B) clamped to [0, R] as sca_wer_counts clamps it (a reference may be empty).
 * Per clip b, with lp = clamp(log_softmax(logits[b, t]), -100, 0), the log-probabilities of
 * sca_ctc_loss_fwd:
 *   ll_n   = the exact CTC log-likelihood of hypothesis n over the frames [0, in_len_b): the
 *            alpha recursion of the CTC loss WITHOUT its rule T_b = max(in_len, 1, S_b).  A
 *            hypothesis that does not fit (len + adjacent repeats > in_len) has ll = -inf; the
 *            empty hypothesis has ll = sum_t lp[t, 0], 0 for in_len = 0.
 *   V      = the valid entries: n < count and ll_n finite (a NaN ll counts as valid, so that it
 *            reaches the loss).  post_n = softmax over V of posterior_scale * ll_n, 0 outside V.
 *   err_n  = num_del + num_ins + num_sub of sca_wer_counts with reference ref_b and hypothesis
 *            h_n: the same device code as the WER kernel and sca_nbest_mbr (costs 3 / 3 / 4 and
 *            the back-trace's order of preference: not Levenshtein's counts).
 *   ebar_b = the mean of err over V;  d_n = err_n - ebar_b;  risk_b = sum_V post_n err_n;
 *   loss_b = sum_V post_n d_n;  loss = (1 / B) sum_b loss_b; a clip with empty V contributes 0.
 * Gradient, with w_n = (dloss / B) posterior_scale post_n (d_n - sum_V post_m d_m) (the centred
 * form: a list whose error counts are all equal has every w_n exactly 0):
 *   d loss / d lp[t, c] = sum_n w_n occ_n(t, c),  occ_n(t, c) = sum over the states s of h_n with
 *   label c of exp(alpha_n[t, s] + beta_n[t, s] - lp[t, c] - ll_n), followed by the gate of the
 *   clamp and the log-softmax backward as in sca_ctc_loss_bwd.  Rows t >= in_len_b, and clips
 *   with at most one valid entry, are written as zeros; every element of dlogits is written.
 * Outputs of fwd: loglik (B, N) (-inf for entries >= count and for those that do not fit),
 * posterior (B, N), errors (B, N) int32 (0 for entries >= count), risk (B), loss (1).  ws:
 * sca_mwer_workspace_floats(B, N, T, H) floats, kept between the forward and the backward (row
 * statistics, alpha, beta, ll, w).  bwd: dloss (1 float, device).
 * Limits, validated before any GPU call: 1 <= B <= 65535, T >= 1, C <= SCA_CTC_MAX_C,
 * 1 <= N <= SCA_CTC_MAX_BEAM, 1 <= H, R <= SCA_WER_MAX_LEN.  Tokens and lengths are clamped
 * in-kernel only to stay in bounds; entries >= count may hold anything and are ignored.  Tokens
 * are class ids in [1, C): no decoder emits the blank; a token 0 is treated as one more blank
 * state (no skip transition into it, its occupancy counted with the blank's).
 * Three launches forward (row statistics; one launch with alpha and beta, one wave64 per (clip,
 * entry, direction), beside the error count of every (clip, entry), one workgroup each; the
 * per-clip statistics and the loss, one workgroup for B <= 64, else four clips per workgroup and
 * one more launch for the fixed-order sum over the clips) and one backward (one workgroup per
 * logits row: one dense gradient pass for the N
 * hypotheses).  Nothing allocates, copies or synchronises (capturable).  No float atomics:
 * every reduction over entries, states and clips runs in a fixed order, so a replayed capture is
 * bitwise the eager call.                                                                    */
long sca_mwer_workspace_floats(int B, int N, int T, int H);
int sca_mwer_fwd(const float* logits, const int* in_len, const int* tokens, const int* out_len, const int* count,
                 const int* ref, const int* ref_len, int B, int N, int T, int C, int H, int R, float posterior_scale,
                 float* loglik, float* posterior, int* errors, float* risk, float* loss, float* ws, void* stream);
int sca_mwer_bwd(const float* logits, const int* in_len, const int* tokens, const int* out_len, const int* count,
                 int B, int N, int T, int C, int H, const float* dloss, const float* ws, float* dlogits,
                 void* stream);

/* ---- training: MWER with the reference in the list, the gloss model's prior, G heads --------
 * sca_mwer_heads_fwd / sca_mwer_heads_bwd: the loss above over the logits of G heads in one
 * call, 1 <= G <= SCA_EVAL_MAX_HEADS (fp32 (B, T, C) per head, by value in `heads`), optionally
 * with the clip's reference as one more entry of its list and with sca_nbest_rescore's prior
 * inside the posterior.  Inputs per head g and clip b: the list tokens (G, B, N, H), out_len
 * (G, B, N), count (G, B); in_len (B) and the references ref (B, R), ref_len (B) are shared by
 * the heads.  lp, ll_n, the fit rule, err_n and the clamping of lengths are exactly those of
 * sca_mwer_fwd.
 *   Slots: M = N + 1 with with_ref != 0, else M = N.  Slots 0 .. N-1 are the list's.  Slot N is
 *     the reference of clip b: its labels ref[b, :ref_len_b], ll_N its exact CTC log-likelihood
 *     over [0, in_len_b) (the same recursion; the reference may be longer than H: the lattice row
 *     has 2 max(H, R) + 1 states), err_N = 0.
 *   Slot N is valid iff ll_N is finite or NaN, as for any entry, AND the reference is not in the
 *     list already: no entry n < count has err_n == 0.  Under the alignment's costs an error
 *     count of 0 holds exactly when the two sequences are equal, and a list that held the
 *     reference twice would double its mass.  ref_valid (G, B) int32 says whether slot N is in V
 *     (0 without with_ref).  loglik[.., N] is the reference's ll whenever it fits and -inf
 *     otherwise, also where the slot is a duplicate and not in V.  Where in_len >= ref_len +
 *     adjacent repeats, so that the CTC loss's rule T_b = max(in_len, 1, S_b) changes nothing,
 *     it is -nll of sca_ctc_loss_fwd for the clip.
 *   Prior: lmterm_n = lm_weight * lm(h_n) + length_bonus * len(h_n), lm(h) being
 *     sca_nbest_rescore's and the same device code: class 0 is the boundary, lm(empty) =
 *     lm[0, 0], lm = NULL means lm(h) = 0.  It applies to the reference slot too.  The term is
 *     computed and added only with lm != NULL or length_bonus != 0: otherwise it is +0.0f.
 *   z_n = posterior_scale * (ll_n + lmterm_n), post = softmax over V of z; ebar, d_n, risk,
 *     loss_b and w_n as above over the enlarged V; loss (G): one mean over the B clips per head.
 *     The prior is a constant of the posterior, so the gradient formula is unchanged; the
 *     occupancies of slot N come from the reference's own lattice and are accumulated last.  A
 *     clip whose only valid slot is the reference has zero rows.
 * Outputs of fwd: loglik, posterior (G, B, M) fp32, errors (G, B, M) int32 (0 in slot N),
 * ref_valid (G, B) int32, risk (G, B), loss (G).  bwd: dloss (G floats, device), dlogits: the G
 * tensors (B, T, C) by value in a sca_mwer_grads; every element is written.  ws:
 * sca_mwer_heads_workspace_floats(G, B, N, T, H, R, with_ref) floats (0 for sizes < 1), kept
 * between the forward and the backward; bwd takes the forward's G, sizes and with_ref.
 * With lm_weight = 0, length_bonus = 0 and a finite table every output is bitwise the lm = NULL
 * call's; without with_ref and with lm = NULL, weight 0 and bonus 0, head g's outputs are
 * bitwise sca_mwer_fwd / sca_mwer_bwd's on heads->logits[g]; head g of a grouped call is
 * bitwise the G = 1 call on that head.
 * Limits, validated before any GPU call: those of sca_mwer_fwd with G B <= 65535, and finite
 * lm_weight and length_bonus; N = 32 with the reference gives 33 slots.  The launches are
 * sca_mwer_fwd's, over (head, clip) pairs p = g B + b: three forward (four above 64 pairs), the
 * reference slot one more x-index of the second and the prior computed beside the alignment, not
 * on the recursions' chain; one backward.  The list is never copied.  Nothing allocates, copies
 * or synchronises (capturable); no float atomics, every reduction runs in a fixed order, and a
 * replayed capture is bitwise the eager call.                                                */
typedef struct {
  float* dlogits[SCA_EVAL_MAX_HEADS]; /* entries [G, 8) are ignored */
} sca_mwer_grads;
long sca_mwer_heads_workspace_floats(int G, int B, int N, int T, int H, int R, int with_ref);
int sca_mwer_heads_fwd(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                       const int* out_len, const int* count, const int* ref, const int* ref_len, int B, int N, int T,
                       int C, int H, int R, int with_ref, const float* lm, float lm_weight, float length_bonus,
                       float posterior_scale, float* loglik, float* posterior, int* errors, int* ref_valid,
                       float* risk, float* loss, float* ws, void* stream);
int sca_mwer_heads_bwd(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                       const int* out_len, const int* count, const int* ref, const int* ref_len, int B, int N, int T,
                       int C, int H, int R, int with_ref, const float* dloss, const float* ws,
                       const sca_mwer_grads* dlogits, void* stream);

/* ---- the backoff n-gram gloss model: a sparse trigram for the second pass and MWER -----------
 * sca_ngram_lm: an ARPA-style backoff model of order 1 to 3 over the C classes, natural-log
 * fp32 values, on the device as a sorted trie.  Class 0 is the sentence boundary on both sides:
 * <s> as context, </s> as predicted word.  Passed by pointer; the entry points copy the struct
 * by value into the kernel arguments, the arrays stay the caller's.
 *   unigrams  uni_lp[C], uni_bo[C]
 *   bigrams   bi_ptr[C + 1]: the CSR row pointer by context v; bi_tok[n_bi]: the successors w,
 *             strictly ascending inside a row; bi_lp[n_bi], bi_bo[n_bi]
 *   trigrams  tri_ptr[n_bi + 1]: the CSR row pointer over the bigram entry of (u, v);
 *             tri_tok[n_tri]: the successors w, strictly ascending; tri_lp[n_tri]
 * Arrays of orders above `order` may be NULL (and arrays of a count of 0).
 *
 * For a labelling h of len tokens, path = [0] + h + [0] and
 *   lm(h) = sum_{k = 1 .. len + 1} p(path[k] | context),
 * so lm(empty) = p2(0 | 0) (order 1: uni_lp[0]).  The term at k uses the two previous path
 * elements with order = 3 and k >= 2, one at k = 1 and everywhere with order = 2, none with
 * order = 1.  The backoff rule, in fp32 with the additions in exactly this order:
 *   p3(w | u, v) = tri_lp[u, v, w] if stored; else bi_bo[u, v] + p2(w | v) if the bigram (u, v)
 *                  is stored; else p2(w | v)
 *   p2(w | v)    = bi_lp[v, w] if stored; else uni_bo[v] + uni_lp[w]
 *   p1(w)        = uni_lp[w]
 * A look-up is a binary search inside one row: a trigram term needs at most three, (u, v) in
 * row u, w in that entry's trigram row, w in row v.  Tokens are clamped into [0, C) only to stay
 * in bounds, and every row range is clamped into [0, n_bi] or [0, n_tri] before the search: a
 * corrupt table can neither read out of bounds nor loop.  The terms of one labelling are summed
 * by the lane stride and the butterfly of the dense table's sum, so an order-2 model whose dense
 * form holds fp32(uni_bo[v] + uni_lp[w]) in the backed-off cells gives bitwise the dense result.
 *
 * sca_nbest_rescore_ngram is sca_nbest_rescore, and sca_mwer_heads_fwd_ngram is
 * sca_mwer_heads_fwd, with `const sca_ngram_lm* lm` (NULL: lm(h) = 0) in place of the dense
 * table (and its C): lm(h) enters total and lmterm as lm_weight * lm(h) + length_bonus * len.
 * sca_mwer_heads_bwd serves both forwards (the prior does not reach the gradient) and the
 * workspace size is unchanged.  Validated before any GPU call: order in 1..3, 1 <= C <=
 * SCA_CTC_MAX_C (for MWER: C equal to the logits'), n_bi, n_tri >= 0, non-NULL arrays for the
 * orders in use, finite lm_weight and length_bonus, and the limits of the dense entry point.
 * Neither allocates, copies or synchronises (capturable).  With lm_weight = 0, length_bonus = 0
 * and finite stored values every output is bitwise the lm = NULL call's.  The fused beam search
 * takes the dense table only: its frame scans a dense row per beam.                          */
typedef struct {
  int order, C, n_bi, n_tri;
  const float* uni_lp;
  const float* uni_bo;
  const int* bi_ptr;
  const int* bi_tok;
  const float* bi_lp;
  const float* bi_bo;
  const int* tri_ptr;
  const int* tri_tok;
  const float* tri_lp;
} sca_ngram_lm;
int sca_nbest_rescore_ngram(const int* tokens, const int* out_len, const float* score, const int* count, int G,
                            int B, int N, int T, const sca_ngram_lm* lm, float lm_weight, float length_bonus,
                            float posterior_scale, float* total, float* posterior, int* order, void* stream);
int sca_mwer_heads_fwd_ngram(const sca_decode_heads* heads, int G, const int* in_len, const int* tokens,
                             const int* out_len, const int* count, const int* ref, const int* ref_len, int B, int N,
                             int T, int C, int H, int R, int with_ref, const sca_ngram_lm* lm, float lm_weight,
                             float length_bonus, float posterior_scale, float* loglik, float* posterior, int* errors,
                             int* ref_valid, float* risk, float* loss, float* ws, void* stream);

/* ---- evaluation: CTC forced alignment (gloss spans and confidences) -----------------------
 * The best single path of G heads' logits through given label sequences: for every (head g,
 * clip b) the frames at which each label is emitted.  Logits as for the decoders (fp32
 * (B, T, C) per head, by value in `heads`, blank = class 0); in_len (B) int32, clamped
 * in-kernel to [0, T].  labels_per_head = 0: labels (B, S) int32 / lab_len (B) are shared by
 * all heads (the references); labels_per_head = 1: labels (G, B, S) / lab_len (G, B) (each
 * head's own hypotheses: the grouped decoders' tokens / out_len as they are).  lab_len is
 * clamped to [0, S]; label values are clamped into [1, C) only to stay in bounds (the caller
 * validates).  1 <= G <= SCA_EVAL_MAX_HEADS, B >= 1, any T >= 1, C <= SCA_CTC_MAX_C,
 * 0 <= S <= SCA_CTC_MAX_S.
 *
 * Per (g, b), T_b / S_b the clamped lengths, lp = log_softmax(logits[b, t]) (no clamp):
 * L = 2 S_b + 1 extended states, blank at the even states and label j at state 2 j + 1.
 * Viterbi in log space: v_0[0] = lp_0[0], v_0[1] = lp_0[l_0], every other state -inf;
 *   v_t[s] = lp_t[ext(s)] + max(v_{t-1}[s], v_{t-1}[s-1], v_{t-1}[s-2])
 * the third term only for odd s >= 3 whose label differs from the label of state s - 2.
 * Ties: the predecessor is s unless s - 1 is strictly greater, and s - 2 only if it is strictly
 * greater than both.  The path ends in state L - 1 only if v[L-1] > v[L-2], otherwise in L - 2
 * (L = 1: state 0).  The clip is infeasible when that value is -inf: T_b < S_b + the number of
 * adjacent equal labels, or T_b = 0 with S_b > 0.
 *
 * Outputs, every element written by every call:
 *   frame_label (G, B, T) int32  the index j of the label emitted at frame t; -1 at blank
 *                                frames and at t >= T_b
 *   spans (G, B, S, 2) int32     [start, end) frames of label j; (0, 0) for j >= S_b
 *   conf (G, B, S) fp32          the mean of exp(lp_t[l_j]) over the span's frames; 0 for j >= S_b
 *   score (G, B) fp32            the path's log-probability; 0 for T_b = S_b = 0
 * An infeasible clip has score = -inf, frame_label = -1 and spans and conf zero.
 *
 * ws: sca_ctc_align_workspace_bytes(G, B, T, S) bytes (0 for unsupported sizes), 8-byte
 * aligned: the row statistics and two bits of back-pointer per (frame, state).  Two launches
 * whatever G and B are: the row statistics of all G B T rows, then one workgroup per
 * (head, clip); no allocation, copy or synchronisation (capturable).  Head g's results are
 * bitwise those of a G = 1 call on heads->logits[g] with its labels.                        */
long sca_ctc_align_workspace_bytes(int G, int B, int T, int S);
int sca_ctc_align_heads(const sca_decode_heads* heads, int G, const int* in_len, const int* labels,
                        const int* lab_len, int labels_per_head, int B, int T, int C, int S, int* frame_label,
                        int* spans, float* conf, float* score, void* ws, void* stream);

/* ---- evaluation: ensemble of the heads' posteriors -----------------------------------------
 * out (B, T, C) fp32 = the normalised log-probabilities of the weighted mean of G heads'
 * posteriors, 1 <= G <= SCA_EVAL_MAX_HEADS: the tensor the multi-stream recognisers decode
 * next to the single heads.  Logits as for the decoders: fp32 (B, T, C) per head, contiguous,
 * the G device pointers by value in `heads`; the G weights by value in `weights` (finite,
 * positive; entries [G, 8) are ignored), normalised here in double: W_g = w_g / sum w.  No
 * device table, nothing to upload: capturable.  Any C >= 1 and any B T >= 1; `out` is none of
 * the inputs.  Every element of `out` is written by every call.
 *
 * Per row (b, t), lp_g[c] = x_g[c] - logsumexp_c x_g (the decoders' row pass: max, then the sum
 * of exp(x - max)):
 *   mode 0 ("prob"), the arithmetic mean of the posteriors:
 *     out[c] = log sum_g W_g exp(lp_g[c]), computed as M + log sum_g exp(a_g - M) with
 *     a_g = lp_g[c] + log W_g and M = max_g a_g: logits at the heads' clamp (+-50) neither
 *     overflow nor collapse to -inf.
 *   mode 1 ("logprob"), the log-linear (geometric) mean, renormalised:
 *     u[c] = sum_g W_g lp_g[c], summed for g = 0 .. G - 1 in this order;
 *     out[c] = u[c] - logsumexp_c u.
 * Both modes give normalised log-probabilities, and with G = 1 both give the row's log_softmax.
 * Specified for finite logits (what RecognitionHead produces).
 *
 * One launch whatever G is: one wave per row, four rows per workgroup; 16-byte loads and stores
 * where every head's row and the output row start on a 16-byte boundary and C % 4 == 0, scalar
 * ones otherwise.  No atomics and a fixed order of every sum: a row's result depends on
 * nothing but the row (not on B, T or the rows beside it), and a replayed capture is bitwise
 * the eager call.                                                                          */
typedef struct {
  float w[SCA_EVAL_MAX_HEADS]; /* entries [G, 8) are ignored */
} sca_ensemble_weights;
int sca_ensemble_log_probs(const sca_decode_heads* heads, int G, const sca_ensemble_weights* weights, int mode,
                           int B, int T, int C, float* out, void* stream);

/* The vector-Jacobian product of sca_ensemble_log_probs: dlogits[g] (B, T, C) fp32 =
 * (d out / d x_g)^T dout for the members of one forward, in one launch.  heads, G, weights (again
 * normalised here in double, exactly as the forward does), mode, B, T, C: the forward's; out:
 * the forward's output; dout (B, T, C): the incoming gradient, contiguous.  The weights are host
 * constants without a gradient.  dlogits: up to G device pointers by value (entries [G, 8) are
 * ignored).  A null entry means "this member takes no gradient": nothing of it is computed or
 * written; with every entry null nothing is launched.  Every element of a non-null entry is
 * written.
 *
 * Per row, p_g = softmax(x_g), lp_g = log p_g, q = exp(out):
 *   mode 0:  r_g[c] = exp(lp_g[c] + log W_g - out[c])   (member g's responsibility for class c;
 *            <= 1 by construction, so nothing overflows at the heads' clamp)
 *            dx_g[k] = r_g[k] dout[k] - p_g[k] sum_c r_g[c] dout[c]
 *   mode 1:  du[c] = dout[c] - q[c] sum_c' dout[c']
 *            dx_g[k] = W_g du[k]
 *            This is the form implemented: the chain through log_softmax(x_g) adds
 *            - W_g p_g[k] sum_c du[c], and that sum is identically 0 because sum q = 1.  The
 *            members are not read in this mode.
 * A row with dout = 0 gets gradients that compare == 0 in both modes.  In mode 0 the members'
 * row statistics (max, log-sum-exp) are recomputed as the forward computes them; nothing is
 * saved between the two calls but `out`.
 *
 * The forward's shape: one wave per row, four rows per workgroup; 16-byte loads and stores where
 * every row involved (the members, out, dout and every non-null gradient) starts on a 16-byte
 * boundary and C % 4 == 0, scalar ones otherwise.  No atomics, no LDS, no barrier, a fixed order
 * of every sum: a row's gradients depend on nothing but the row, and a replayed capture is
 * bitwise the eager call.  Nothing allocates, copies or synchronises (capturable).
 * SCA_ERR_ARG before any GPU call: the forward's checks on heads, G, weights, mode and sizes; a
 * null out, dout or dlogits; out == dout; a non-null gradient tensor that is out, dout, a member
 * or another gradient tensor.                                                              */
typedef struct {
  float* dlogits[SCA_EVAL_MAX_HEADS]; /* entries [G, 8) are ignored; NULL: no gradient for this member */
} sca_ensemble_grads;
int sca_ensemble_log_probs_bwd(const sca_decode_heads* heads, int G, const sca_ensemble_weights* weights,
                               int mode, int B, int T, int C, const float* out, const float* dout,
                               const sca_ensemble_grads* dlogits, void* stream);

/* The same ensemble with learned weights: weight_logits (G) fp32 on the device are G unconstrained
 * scores theta, and W = softmax(theta) takes the place of the host weights above (positive and
 * normalised by construction; theta = 0 gives equal weights).  The kernel reads theta from memory,
 * so nothing about the weights is frozen in a captured graph: a replay after an optimizer step or
 * a load_state_dict on theta computes with the new weights.  Every wave computes
 * log W_g = (theta_g - max theta) - log sum_g exp(theta_g - max theta) and W_g = exp(log W_g) once
 * (G wave-uniform loads), the same function in the forward and the backward; the row arithmetic,
 * the launch shape and the guarantees are those of sca_ensemble_log_probs.  Specified for finite
 * theta.  SCA_ERR_ARG before any GPU call: the checks of sca_ensemble_log_probs on heads, G, mode
 * and sizes; a null weight_logits or out; weight_logits that is out or a member.
 *
 * sca_ensemble_log_probs_dw_bwd: the members' gradients are exactly those of
 * sca_ensemble_log_probs_bwd with W from theta (a null entry of dlogits is skipped), and
 * dweight_logits (G) fp32, or NULL for "theta takes no gradient", is d theta summed over all
 * B T rows.  Per row, with r_g, du and q as above and D = sum_c dout[c]:
 *   mode 0:  d theta_g += s_g - W_g D,  s_g = sum_c r_g[c] dout[c]
 *            (the s_g of the members' gradient, here formed for every member, also one whose
 *            dlogits entry is null)
 *   mode 1:  d theta_g += W_g sum_c du[c] (lp_g[c] - out[c])
 *            (out in the place of u is exact because sum_c du = 0; with dweight_logits the
 *            members and their row statistics are read in this mode too, without it still not)
 * sum_g d theta_g = 0 up to rounding; a row with dout = 0 contributes exactly 0; with G = 1 the
 * entry writes dweight_logits[0] = 0 (a 4-byte memset) and computes nothing for it.
 *
 * The sum over the rows takes two launches.  The row kernel (one wave per row as above, no LDS, no
 * barrier) stores its row's G partials into ws (B T, G) with plain stores; then one workgroup
 * sums them in a fixed order: thread t adds the rows t, t + 256, ... ascending, and an LDS tree
 * adds the 256 threads.  No float atomics and no counter: d theta depends on the partials alone,
 * and a replayed capture is bitwise the eager call.  ws: sca_ensemble_log_probs_dw_workspace_bytes
 * (G, B, T) bytes (0 for G = 1 or sizes out of range), needed only with dweight_logits and
 * G >= 2.  With dweight_logits NULL and every dlogits entry null nothing is launched.
 * SCA_ERR_ARG before any GPU call: the forward's checks; a null out, dout or dlogits; out ==
 * dout; weight_logits that is out or dout; a null ws where it is needed; a non-null gradient
 * tensor, dweight_logits or ws that is out, dout, weight_logits, a member or another of them.  */
int sca_ensemble_log_probs_dw(const sca_decode_heads* heads, int G, const float* weight_logits, int mode, int B,
                              int T, int C, float* out, void* stream);
long sca_ensemble_log_probs_dw_workspace_bytes(int G, int B, int T);
int sca_ensemble_log_probs_dw_bwd(const sca_decode_heads* heads, int G, const float* weight_logits, int mode,
                                  int B, int T, int C, const float* out, const float* dout,
                                  const sca_ensemble_grads* dlogits, float* dweight_logits, void* ws, void* stream);

/* SeqKD over R rows of C logits (student, teacher): columns [start, C) only (use_blank=False
 * -> start 1), temperature temp:
 *   loss = clamp(weight * temp^2 * (1/R) * sum_rows KL(softmax(q/temp) || log_softmax(s/temp)),
 *                lo, hi)
 * (KLDivLoss 'batchmean' over the .view(-1, C') rows).  ws: sca_seqkd_workspace_floats(R).
 * bwd writes d loss / d student (dstudent) and/or d loss / d teacher (dteacher; NULL when
 * the teacher is detached, as the reference does), zeros in columns < start.              */
long sca_seqkd_workspace_floats(int R);
int sca_seqkd_fwd(const float* student, const float* teacher, int R, int C, int start, float temp, float weight,
                  float lo, float hi, float* loss, float* ws, void* stream);
int sca_seqkd_bwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                  const float* dloss, const float* ws, float* dstudent, float* dteacher, void* stream);
/* Valid-frame variants (see sca_softmax_rows_valid_fwd): the R rows are (b, t) with t = r % T
 * (R a multiple of T); only rows with t < nv contribute, the divisor is (R / T) * nv, and the
 * backward writes exact zeros into the rows with t >= nv.  Same fixed-order reduction (the
 * skipped rows add exact zeros), same workspace.                                           */
int sca_seqkd_valid_fwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                        float weight, float lo, float hi, float* loss, float* ws, int T, const int* valid_frames,
                        int shift, void* stream);
int sca_seqkd_valid_bwd(const float* student, const float* teacher, int R, int C, int start, float temp,
                        const float* dloss, const float* ws, float* dstudent, float* dteacher, int T,
                        const int* valid_frames, int shift, void* stream);

/* Ensemble distillation (no counterpart): SeqKD of S students, 1 <= S <=
 * SCA_DISTILL_MAX_STUDENTS, against the ensemble of G members, 1 <= G <= SCA_EVAL_MAX_HEADS, in
 * one call.  The teacher is formed on the fly and never stored.  By definition
 *   losses[s] = sca_seqkd_fwd(students[s], e, R = B T, C, start, temp, weight[s], lo, hi)
 *   e         = sca_ensemble_log_probs(members, G, W, mode)
 * where per row only softmax(e[start:] / temp) matters: in mode 1 the outer normalisation of
 * u = sum_g W_g lp_g is not computed, and with G = 1 the member's logits are read as the teacher's
 * (its log-sum-exp cancels too) with the row arithmetic of sca_seqkd_*, so that the call is then
 * BITWISE sca_seqkd_fwd / _bwd (with valid_frames: the _valid pair) once per student.
 * Weights: exactly one of `weights` (host, normalised in double as sca_ensemble_log_probs does)
 * and `weight_logits` ((G) fp32 on the device, W = softmax of it, read by every wave as
 * sca_ensemble_log_probs_dw does, so a captured graph follows an update).  A student may be one
 * of the members.  valid_frames: NULL, or the device scalar of the *_valid entries with `shift`:
 * rows with t >= nv = clamp(*valid_frames >> shift, 1, T) contribute exact zeros, the divisor is
 * B nv and the backward writes exact zeros into those rows.
 * The teacher is detached: the backward writes, for every non-NULL dstudents->dlogits[s],
 *   dstudent_s = dlosses[s] gate_s weight[s] temp / rows (softmax(s / temp) - q)  in columns >=
 * start and zeros below, gate_s being the clamp gate the forward left in ws; a NULL entry is
 * skipped (nothing of it is computed or written) and with every entry NULL nothing is launched.
 * Neither the members nor weight_logits take a gradient.
 * One wave64 per (row, student); 16-byte loads where every row involved starts on a 16-byte
 * boundary and C % 4 == 0 (G >= 2), scalar loads otherwise; no atomics, every sum in a fixed
 * order, a row's result depends on the row alone; nothing allocates, copies or synchronises, so
 * the calls are capturable and a replay is bitwise the eager call.  fwd: two launches (the rows,
 * then one finalize for all S); bwd: one.  ws: sca_distill_heads_workspace_floats(S, G, B, T)
 * floats (0 for arguments out of range), written by fwd and read by bwd: per student the row
 * losses, the row statistics and the gate, and for G >= 2 the members' row statistics.
 * SCA_ERR_ARG before any GPU call: the ensemble entries' checks on members, G, the weights and
 * mode; S out of range; a NULL student, losses, dlosses, dstudents or ws; temp <= 0; start outside
 * [0, C); with valid_frames, shift outside [0, 30]; both or neither weight source; losses, ws (fwd)
 * or a non-NULL dstudent (bwd) that is a member, a student, weight_logits, valid_frames, dlosses,
 * ws or another output.                                                                    */
#define SCA_DISTILL_MAX_STUDENTS 8
typedef struct {
  const float* logits[SCA_DISTILL_MAX_STUDENTS]; /* entries [S, 8) are ignored */
  float weight[SCA_DISTILL_MAX_STUDENTS];
} sca_distill_students;
typedef struct {
  float* dlogits[SCA_DISTILL_MAX_STUDENTS]; /* entries [S, 8) are ignored; NULL: no gradient for this student */
} sca_distill_grads;
long sca_distill_heads_workspace_floats(int S, int G, int B, int T);
int sca_distill_heads_fwd(const sca_decode_heads* members, int G, const sca_ensemble_weights* weights,
                          const float* weight_logits, int mode, const sca_distill_students* students, int S, int B,
                          int T, int C, int start, float temp, float lo, float hi, const int* valid_frames, int shift,
                          float* losses, float* ws, void* stream);
int sca_distill_heads_bwd(const sca_decode_heads* members, int G, const sca_ensemble_weights* weights,
                          const float* weight_logits, int mode, const sca_distill_students* students, int S, int B,
                          int T, int C, int start, float temp, const int* valid_frames, int shift,
                          const float* dlosses, const float* ws, const sca_distill_grads* dstudents, void* stream);

/* torch.clamp(x, lo, hi) over n elements (dy == NULL; a NaN stays a NaN), or its backward
 * dx = dy * [lo <= x <= hi] */
int sca_clamp(const float* x, float* y, const float* dy, float* dx, long n, float lo, float hi, void* stream);

/* One time step of a (bi)directional LSTM cell (AlignmentModule's nn.LSTM,
 * model/alignment_module.py:24-30), batch-major, both directions per launch (direction 1
 * walks t = T-1 .. 0); gate order i, f, g, o.  The projections around it are sca_gemm
 * launches.  D = ndir.  fwd: gates (B, D*4H) pre-activations of this step -> act
 * (B, T, D*4H), c / y (B, T, D*H), and hp (B, T, D*H) = the hidden state each step reads
 * (h_{t-1} for direction 0, h_{t+1} for direction 1; zero-filled by the caller).
 * bwd (step k walks t = T-1-k / t = k): dh (B, D*H) = dY_t + dG_{t'} W_hh (NULL at k = 0,
 * where dy (B, T, D*H) is read instead), dc (B, D*H) carried in place, dg (B, T, D*4H) the
 * gate pre-activation gradients.                                                          */
int sca_lstm_cell_fwd(const float* gates, float* act, float* c, float* y, float* hp, int B, int T, int H, int ndir,
                      int step, void* stream);
int sca_lstm_cell_bwd(const float* dh, const float* dy, const float* act, const float* c, float* dc, float* dg,
                      int B, int T, int H, int ndir, int step, void* stream);
/* Valid-frame variants (see sca_softmax_rows_valid_fwd).  The caller still issues T steps (the
 * launch count of a captured graph is fixed).  fwd, frame t >= nv: c = y = 0, zero
 * activations, and the hp of the frame the direction visits next = 0 — so direction 1 reaches
 * t = nv-1 with zero state, which is step 0 of an unpadded run (the recurrent GEMM over h = 0
 * gives b_hh + G_t in both).  bwd, frame t >= nv: dg = 0, dc = 0, the incoming dh is ignored;
 * at t = nv-1 the step then sees dh = dY_t + 0 and dc = 0, again the unpadded step 0.      */
int sca_lstm_cell_valid_fwd(const float* gates, float* act, float* c, float* y, float* hp, int B, int T, int H,
                            int ndir, int step, const int* valid_frames, int shift, void* stream);
int sca_lstm_cell_valid_bwd(const float* dh, const float* dy, const float* act, const float* c, float* dc,
                            float* dg, int B, int T, int H, int ndir, int step, const int* valid_frames, int shift,
                            void* stream);

/* ---- training update: gradient clip + Adam over every parameter tensor in two launches ----
 * Replaces clip_grad_norm_(model.parameters(), max_norm) + optimizer.step() (opt.py:34-35)
 * for the torch.optim.Adam of optimizer.py:49-66, and the NaN-loss skip of opt.py:32-37
 * without its host sync.  The kernels read four tables in DEVICE memory:
 *   tensors  one entry per parameter tensor that has a gradient
 *   chunks   the tensors cut into pieces of a fixed size (the last piece of a tensor may be
 *            shorter; no piece spans two tensors); workgroups stride over this list
 *   groups   the hyper-parameters of each parameter group (doubles, as torch keeps them)
 *   state    step counter, skip flag, and the last step's gradient norm and clip coefficient
 * partials: workspace of sca_optim_blocks(max_blocks, nchunks) floats, written by
 * sca_optim_grad_sqnorm and read by the launch that follows it with the same nchunks and
 * max_blocks (0: the default grid cap, 8 workgroups per CU).  Sums run in a fixed order with
 * no atomics: results are bitwise reproducible for a given table and max_blocks.          */
typedef struct {
  float* p;                /* parameter, numel floats                                      */
  float* g;                /* its gradient (read; scaled in place by sca_optim_scale_grads) */
  float* exp_avg;          /* first moment                                                 */
  float* exp_avg_sq;       /* second moment                                                */
  float* max_exp_avg_sq;   /* amsgrad: running maximum of the second moment, else NULL     */
  long numel;
  int group;               /* index into the group table                                   */
  int t0;                  /* state.step before this tensor's first update: its own step
                              (torch keeps one per parameter) is state.step - t0           */
} sca_optim_tensor;

typedef struct {
  int tensor;              /* index into the tensor table                                  */
  int len;                 /* elements in this chunk                                       */
  long offset;             /* first element, from the tensor's base                        */
} sca_optim_chunk;

typedef struct {
  double lr, beta1, beta2, eps, weight_decay;
} sca_optim_group;

typedef struct {
  int step;                /* updates applied so far                                       */
  int skipped;             /* 1 when the last call saw a non-finite loss                   */
  float grad_norm;         /* total 2-norm of the last call's gradients, before clipping   */
  float clip_coef;         /* min(1, max_norm / (grad_norm + 1e-6)); 1 with clipping off   */
} sca_optim_state;

int sca_optim_blocks(int max_blocks, int nchunks);
/* Pass 1: partials[w] = workgroup w's sum of g^2; workgroup 0 also reads *loss (device
 * scalar, or NULL), sets state.skipped = !isfinite(loss) and increments state.step when not
 * skipped.                                                                                */
int sca_optim_grad_sqnorm(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                          int max_blocks, const float* loss, sca_optim_state* state, float* partials,
                          void* stream);
/* Pass 2: grad_norm = sqrt(sum partials), clip_coef (max_norm <= 0: clipping off) stored in
 * state; unless state.skipped, per element with t = state.step - t0 (torch.optim.Adam with
 * L2 weight decay, optional amsgrad through max_exp_avg_sq):
 *   g' = clip_coef g + wd p ; m += (1 - b1)(g' - m) ; v = b2 v + (1 - b2) g'^2
 *   p -= lr / (1 - b1^t) * m / (sqrt(amsgrad ? vmax = max(vmax, v) : v) / sqrt(1 - b2^t) + eps)
 * The gradient is not written.                                                            */
int sca_optim_adam_step(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                        const sca_optim_group* groups, int max_blocks, float max_norm, sca_optim_state* state,
                        const float* partials, void* stream);
/* After pass 1: g *= clip_coef in place (stand-alone clip_grad_norm_); stores grad_norm and
 * clip_coef in state.                                                                     */
int sca_optim_scale_grads(const sca_optim_tensor* tensors, const sca_optim_chunk* chunks, int nchunks,
                          int max_blocks, float max_norm, sca_optim_state* state, const float* partials,
                          void* stream);
/* Asynchronous host-to-device copy of a table on `stream` (a memcpy node under capture).
 * src must be pinned host memory that is left unmodified and alive for as long as a graph
 * holding the copy can be replayed.                                                       */
int sca_optim_upload(void* dst, const void* src, long bytes, void* stream);

/* ---- finite guard: the NaN / Inf checks of MSCA_Net.forward without their host reads ----
 * sca_finite_scan: ntensors (0..16) contiguous fp32 tensors, given as HOST arrays ptrs /
 * numels (copied into the kernel arguments: no device table).  flags: ntensors 32-bit words in
 * device memory; the call clears them on `stream` (a one-wave launch, not a memset node) and one
 * launch ORs into word t  bit 0 when tensor t holds a NaN,  bit 1 when it holds +-Inf.
 * Elements are classified from their exponent / mantissa bits.  Workgroups stride over
 * SCA_GUARD_CHUNK-element chunks (no chunk spans two tensors), with 16-byte loads between the
 * chunk's first and last 16-byte boundary and 4-byte loads outside; a workgroup issues at
 * most one atomic OR per tensor, none when it found nothing.  numel 0 is legal (no launch
 * when every tensor is empty).  SCA_ERR_ARG: ntensors > 16, a negative numel, a null or
 * misaligned (not 4-byte) pointer with numel > 0.                                          */
#define SCA_GUARD_MAX_TENSORS 16
#define SCA_GUARD_CHUNK 4096
int sca_finite_scan(int ntensors, const float* const* ptrs, const long* numels, unsigned* flags, void* stream);

/* sca_step_report: one small launch after the scan.  report (device, nflags + ndistill + 4
 * 32-bit words) receives
 *   [0, nflags)            the flag words (zeros when flags == NULL: guard switched off)
 *   then, as fp32:         alignment_loss (0 when NULL), fuse_coord_loss, the ndistill
 *                          distillation terms, total_loss, guard
 * with total_loss = fuse_coord_loss + distill[0] + ... in that order (also stored to
 * *total_loss when not NULL) and guard = total_loss when every flag word is zero, NaN
 * otherwise — the scalar FusedAdam.step(loss=...) / sca_optim_grad_sqnorm test, so a flagged
 * tensor that does not feed total_loss skips the update too.  distill: HOST array of device
 * scalars.                                                                                 */
#define SCA_REPORT_MAX_FLAGS 64
#define SCA_REPORT_MAX_DISTILL 8
int sca_step_report(const unsigned* flags, int nflags, const float* alignment_loss, const float* fuse_coord_loss,
                    int ndistill, const float* const* distill, float* total_loss, void* report, void* stream);

/* ---- evaluation step: device-side totals of a whole pass (opt.py:50-128) ----------------- */
/* The state of one evaluation pass, in device memory; all zero = empty (clear it with a memset
 * on the stream).  Only sca_eval_accumulate writes it, so a replayed graph appends where the
 * previous replay stopped.                                                                  */
#define SCA_EVAL_MAX_LOSSES (SCA_REPORT_MAX_DISTILL + 3)
#define SCA_EVAL_LOG_DROPPED 1   /* overflow bit: a clip arrived at or beyond the log's capacity */
#define SCA_EVAL_LOG_TRUNCATED 2 /* overflow bit: a hypothesis was longer than log_width         */
typedef struct {
  int cursor;        /* clips accumulated so far = the log row of the next step's clip 0        */
  int steps;         /* calls accumulated so far                                                */
  int overflow;      /* SCA_EVAL_LOG_* bits                                                     */
  int first_flagged; /* 1 + the index of the first step with a non-zero flag word, 0 = none     */
  int totals[SCA_EVAL_MAX_HEADS][4];      /* per head: sums of (num_del, num_ins, num_sub, num_ref) */
  unsigned flags[SCA_REPORT_MAX_FLAGS];   /* OR of every step's flag words                      */
  double loss_sum[SCA_EVAL_MAX_LOSSES];   /* per loss word, the float64 sum in step order       */
} sca_eval_state;

/* sca_eval_accumulate: one step's hypotheses scored and added to the state, two launches.
 *   tokens (G, B, Hmax) / hyp_len (G, B): the grouped decoders' output (Hmax = their T)
 *   ref (B, Rmax) / ref_len (B): the references, shared by all heads (indexed by clip)
 *   report: the step's sca_step_report buffer: nflags flag words, then nloss fp32 loss words
 *           (alignment_loss, fuse_coord_loss, the distillation terms, total_loss)
 * Launch 1, one workgroup per (head, clip): the counts of sca_wer_counts into counts (G, B, 4)
 * and, with integer atomic adds (they commute: deterministic), into state->totals[g]; when
 * hyp_log is given, clip b's hypothesis goes to log row r = state->cursor + b:
 * hyp_log[r][g][0 .. log_width) int32 zero-padded, hyp_len_log[r][g] its length.  Rows
 * r >= capacity are not written and set SCA_EVAL_LOG_DROPPED; a hypothesis longer than
 * log_width is cut and sets SCA_EVAL_LOG_TRUNCATED.
 * Launch 2, one wave: loss_sum[i] += (double)loss word i, flags[i] |= flag word i,
 * first_flagged, then cursor += B and steps += 1.
 * 1 <= G <= 8, B >= 1, 0 <= Rmax, Hmax <= 128, nflags <= 64, nloss <= 11, capacity >= 0
 * (0: no log; else hyp_log, hyp_len_log and log_width >= 1 are required).                  */
int sca_eval_accumulate(const int* tokens, const int* hyp_len, int G, int B, int Hmax, const int* ref,
                        const int* ref_len, int Rmax, const void* report, int nflags, int nloss, int* counts,
                        sca_eval_state* state, int* hyp_log, int* hyp_len_log, int capacity, int log_width,
                        void* stream);

/* sca_eval_log_alignments: one step's alignments (sca_ctc_align_heads: spans (G, B, S, 2),
 * conf (G, B, S), score (G, B)) appended to a pass's alignment log, one launch.  It reads
 * state->cursor on the device and writes clip b to row r = cursor + b of
 * span_log (capacity, G, log_width, 2) int32, conf_log (capacity, G, log_width) fp32 (columns
 * [S, log_width) zero) and score_log (capacity, G) fp32.  It only READS the state: enqueue it
 * BEFORE the step's sca_eval_accumulate, which advances the cursor, so that a replayed graph
 * appends where the hypothesis log does.  Rows r >= capacity and columns >= log_width are
 * dropped; sca_eval_accumulate raises the overflow bits for the same clips.
 * 1 <= G <= 8, B >= 1, S >= 0, capacity >= 1, log_width >= 1.                               */
int sca_eval_log_alignments(const int* spans, const float* conf, const float* score, int G, int B, int S,
                            const sca_eval_state* state, int* span_log, float* conf_log, float* score_log,
                            int capacity, int log_width, void* stream);

const char* sca_last_error(void);
int sca_version(void);
/* sha256 (first 16 hex digits) of the library sources the binary was built from
 * (the .cpp, .h and .hip files of scattennet_amd/csrc in name order, then this header); the Python binding
 * refuses a library whose digest does not match the sources beside it. */
const char* sca_build_digest(void);

#ifdef __cplusplus
}
#endif
#endif /* SCATTEN_H */
