"""The evaluation step of evaluate_fn (opt.py:50-128) on the device: forward, CTC decoding of
every evaluated head in one grouped launch, WER counts and the pass's totals, with no host
read until the pass is over.

* `ctc_decode_heads_device` (decode.py, exported here too) — the G logit tensors of one forward
  decoded together.
* `EvalState` — the pass's device state (`sca_eval_state`, include/scatten.h): per-head WER
  totals, float64 loss sums, the OR of the finite guard's flag words, and an optional log of
  every hypothesis.  `read()` is the single host read and returns the dict `evaluate_fn`
  returns; `hypotheses()` returns the logged token ids and, with `align=True`, `alignments()`
  each hypothesis's gloss spans and confidences (align.py).
* `eval_step(model, src_input, state, beam_size=5)` — forward (finite check deferred), grouped
  decode, `sca_eval_accumulate`.  No host read; capturable for a fixed (B, T, S) by the rules
  of `train.py`.  It does NOT touch the model's `training` flag: call `model.eval()` first, as
  `evaluate_fn` does (opt.py:62) — a model left in training mode is evaluated with dropout.
* `BucketedEvalStep` — a subclass of `BucketedStep` (bucketed.py), the runner `BucketedTrainStep`
  is built on: batches of any length are padded to a frame bucket, each bucket's step is
  captured on its second use and replayed after, and all buckets append to one `EvalState`.
* `ensembles={output_key: EnsembleSpec}` (ensemble.py) on either: the heads' averaged posterior,
  computed after the forward and decoded, aligned, scored and logged as one more head.
* `rescoring=Rescoring(...)` (nbest.py) on `eval_step` / `BucketedEvalStep`: the n-best decode, the
  bigram rescore and the selection ("score" or "mbr") in place of the 1-best decode; the selected
  hypothesis is aligned, scored and logged like a decoder's.

`{name}wer` keys use the reference's `logits_name` (the output key without "gloss_logits":
"alignment_", "fuse_coord_").  Hypotheses are class ids; the tokenizer, the results JSON and
the logging of `evaluate_fn` stay with the caller.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from .bucketed import BucketedStep, check_buckets
from .align import alignment_lists, ctc_align_heads_device
from .decode import WER_MAX_LEN, ctc_decode_heads_device, wer_from_counts
from .encoder import n_pool_of
from .ensemble import add_ensembles, check_ensembles
from .heads import _dev_i32, labels_2d
from .model import _LOGITS, _students_of, deferred_check, first_error, flag_names
from .nbest import check_rescoring, rescored_decode

MAX_HEADS = L.EVAL_MAX_HEADS


def logits_name(key):
    """opt.py:82: the output key without "gloss_logits"."""
    return key.replace("gloss_logits", "")


def default_heads():
    """The keys evaluate_fn decodes (opt.py:80): those containing "gloss_logits"."""
    return tuple(k for k in _LOGITS if "gloss_logits" in k)


def check_head_keys(heads, what):
    """The decoded heads of a step as a tuple: 1..8 distinct logit keys; None: `default_heads()`."""
    keys = default_heads() if heads is None else tuple(heads)
    if not 1 <= len(keys) <= MAX_HEADS or len(set(keys)) != len(keys):
        raise ValueError(f"{what}: heads must be 1..{MAX_HEADS} distinct keys, got {keys!r}")
    for k in keys:
        if k not in _LOGITS:
            raise ValueError(f"{what}: unknown head {k!r}; the logit keys are {_LOGITS}")
    return keys


def loss_names(students=()):
    """The loss words of `finite_report` that a pass sums, in report order."""
    return ["alignment_loss", "fuse_coord_loss"] + [f"{s}_distill_loss" for s in students] + ["total_loss"]


# ------------------------------------------------------------------------------ the state
def results_from_state(raw, head_keys, loss_keys, flag_keys):
    """The dict evaluate_fn returns (opt.py:101-128), from the raw state of a pass.  Pure host
    function.  `raw`: {"steps", "overflow", "first_flagged", "flags" [>= len(flag_keys)],
    "totals" [>= len(head_keys)][4], "loss_sum" [>= len(loss_keys)] float64}.

    * every loss key: sum of the steps' values / steps (MetricLogger's global_avg over
      `update(k=value)` once per step); `loss`: the same for `total_loss` (opt.py:101)
    * `{logits_name}wer`: metrics.wer_list over all clips of the pass (a zero total counts as 1)
    * `wer`: the minimum over the heads, starting from 200 (opt.py:104, 116-118)

    Raises the reference's ValueError (model/__init__.py:130-235) for the first flagged tensor
    when any step was flagged, RuntimeError when the hypothesis log overflowed."""
    msg = first_error(list(raw["flags"])[:len(flag_keys)], flag_keys)
    if msg is not None:  # raw["first_flagged"] - 1 is the step that was flagged first
        raise ValueError(msg)
    over = int(raw["overflow"])
    if over & L.EVAL_LOG_DROPPED:
        raise RuntimeError("EvalState: the hypothesis log overflowed: more clips arrived than `capacity` rows")
    if over & L.EVAL_LOG_TRUNCATED:
        raise RuntimeError("EvalState: a hypothesis was longer than `log_width` and was cut in the log")
    steps = int(raw["steps"])
    if steps < 1:
        raise RuntimeError("EvalState.read: no step has been accumulated")
    out = {k: float(raw["loss_sum"][i]) / steps for i, k in enumerate(loss_keys)}
    out["loss"] = out["total_loss"]
    out["wer"] = 200
    for g, key in enumerate(head_keys):
        rate = wer_from_counts(torch.as_tensor(np.asarray(raw["totals"][g], dtype=np.int64)).reshape(1, 4))["wer"]
        out[logits_name(key) + "wer"] = rate
        out["wer"] = min(rate, out["wer"])
    return out


class EvalState:
    """The device state of one evaluation pass (`sca_eval_state`, include/scatten.h), shared by
    every `eval_step` of the pass.

    `heads`: the output keys to decode and score, any subset of the five logit keys; default
    the keys evaluate_fn decodes (`alignment_gloss_logits`, `fuse_coord_gloss_logits`).
    `capacity` > 0 attaches a log of `capacity` clips: `hyp_log` (capacity, G, log_width) int32
    zero-padded and `hyp_len_log` (capacity, G); `log_width` is then required (the longest
    hypothesis: the pooled frame count).  `align=True` (needs a log) makes `eval_step` force-align
    every head's hypothesis and attaches `span_log` (capacity, G, log_width, 2) int32, `conf_log`
    (capacity, G, log_width) and `score_log` (capacity, G) fp32, read by `alignments()`.
    `ensembles`: `{output_key: EnsembleSpec}` (ensemble.py); `eval_step` computes each from the
    forward's logits and decodes, aligns, scores and logs it after the plain heads, under its
    `logits_name` (`keys` = `heads` + the ensemble keys is the order of every G above).  The key
    must contain "gloss_logits" and be none of the five logit keys; heads and ensembles together
    are at most 8.  `reset()` clears everything on the current stream."""

    def __init__(self, model, heads=None, capacity=0, log_width=None, align=False, ensembles=None):
        keys = check_head_keys(heads, "EvalState")
        capacity = int(capacity)
        if capacity < 0:
            raise ValueError("EvalState: capacity must not be negative")
        if capacity and (log_width is None or not 1 <= int(log_width) <= WER_MAX_LEN):
            raise ValueError(f"EvalState: a log needs log_width in [1, {WER_MAX_LEN}], got {log_width!r}")
        if align and not capacity:
            raise ValueError("EvalState: align=True needs a log (capacity > 0) to keep the alignments in")
        self.ensembles = check_ensembles(keys, ensembles, "EvalState")
        self.heads = keys
        self.keys = keys + tuple(self.ensembles)  # every decoded tensor: the plain heads, then the ensembles
        self.align = bool(align)
        self.students = list(model._students())
        self.flag_names = flag_names(self.students)
        self.loss_names = loss_names(self.students)
        self.capacity, self.log_width = capacity, int(log_width) if capacity else 0
        self.device = next(model.parameters()).device
        G = len(self.keys)
        self.state = torch.zeros(ctypes.sizeof(L.EvalState) // 8, dtype=torch.int64, device=self.device)
        self.hyp_log = self.hyp_len_log = None
        if capacity:
            self.hyp_log = torch.zeros(capacity, G, self.log_width, dtype=torch.int32, device=self.device)
            self.hyp_len_log = torch.zeros(capacity, G, dtype=torch.int32, device=self.device)
        self.span_log = self.conf_log = self.score_log = None
        if self.align:
            self.span_log = torch.zeros(capacity, G, self.log_width, 2, dtype=torch.int32, device=self.device)
            self.conf_log = torch.zeros(capacity, G, self.log_width, dtype=torch.float32, device=self.device)
            self.score_log = torch.zeros(capacity, G, dtype=torch.float32, device=self.device)

    def reset(self):
        self.state.zero_()
        if self.capacity:
            self.hyp_log.zero_()
            self.hyp_len_log.zero_()
        if self.align:
            self.span_log.zero_()
            self.conf_log.zero_()
            self.score_log.zero_()

    def raw(self):
        """The state as host arrays (one device-to-host copy)."""
        st = L.EvalState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return {"cursor": st.cursor, "steps": st.steps, "overflow": st.overflow, "first_flagged": st.first_flagged,
                "totals": np.ctypeslib.as_array(st.totals).copy(), "flags": list(st.flags),
                "loss_sum": np.ctypeslib.as_array(st.loss_sum).copy()}

    def read(self):
        """The pass's single host read: `results_from_state` of the state."""
        return results_from_state(self.raw(), self.keys, self.loss_names, self.flag_names)

    def hypotheses(self):
        """Per clip, in arrival order: {logits_name: [class ids]} (needs a log: capacity > 0)."""
        if not self.capacity:
            raise RuntimeError("EvalState.hypotheses: no log attached (capacity = 0)")
        n = min(self.raw()["cursor"], self.capacity)
        packed = torch.cat([self.hyp_len_log[:n].unsqueeze(-1), self.hyp_log[:n]], dim=-1).cpu().numpy()
        return [{logits_name(k): packed[r, g, 1:1 + packed[r, g, 0]].tolist() for g, k in enumerate(self.keys)}
                for r in range(n)]

    def alignments(self, frame_scale=1):
        """Per clip, in arrival order: {logits_name: [(class id, start, end, confidence), ...]}, the
        forced alignment of each head's own hypothesis (`align=True`); spans in logit frames times
        `frame_scale`.  One device-to-host copy, like `hypotheses()`."""
        if not self.align:
            raise RuntimeError("EvalState.alignments: the state was built without align=True")
        n = min(self.raw()["cursor"], self.capacity)
        G, W = len(self.keys), self.log_width
        packed = torch.cat([self.hyp_len_log[:n].unsqueeze(-1).double(), self.hyp_log[:n].double(),
                            self.span_log[:n].reshape(n, G, 2 * W).double(), self.conf_log[:n].double(),
                            self.score_log[:n].unsqueeze(-1).double()], dim=-1).cpu().numpy()
        out = []
        for r in range(n):
            clip = {}
            for g, k in enumerate(self.keys):
                row = packed[r, g]
                lists = alignment_lists(row[None, 1:1 + W].astype(np.int64), row[None, 0].astype(np.int64),
                                        row[None, 1 + W:1 + 3 * W].reshape(1, W, 2).astype(np.int64),
                                        row[None, 1 + 3 * W:1 + 4 * W], row[None, 1 + 4 * W], frame_scale)
                clip[logits_name(k)] = lists[0]
            out.append(clip)
        return out


def _references(src_input, B, device):
    lab = labels_2d(src_input, B, "eval_step")
    if lab.shape[1] > WER_MAX_LEN:
        raise ValueError(f"eval_step: references of {lab.shape[1]} tokens exceed the WER kernel's {WER_MAX_LEN}")
    ref_len = torch.as_tensor(src_input["gloss_lengths"]).reshape(-1)
    if ref_len.numel() != B:
        raise ValueError(f"eval_step: gloss_lengths must have {B} entries, got {ref_len.numel()}")
    return _dev_i32(lab, device), _dev_i32(ref_len, device)


def accumulate(state, tokens, lengths, ref, ref_len, report):
    """`sca_eval_accumulate`: tokens (G, B, Hmax) / lengths (G, B) scored against ref (B, Rmax) /
    ref_len (B) (int32, device) and added to `state` with the step's `finite_report`.  Returns
    the step's counts (G, B, 4) int32."""
    G, B, Hmax = tokens.shape
    if G != len(state.keys):
        raise ValueError(f"accumulate: {G} heads decoded, the state holds {len(state.keys)}")
    if ref.dim() != 2 or ref.shape[0] != B:
        raise ValueError(f"accumulate: ref must be ({B}, Rmax), got {tuple(ref.shape)}")
    if Hmax > WER_MAX_LEN or ref.shape[1] > WER_MAX_LEN:
        raise ValueError(f"accumulate: rows of {Hmax} / {ref.shape[1]} tokens exceed the WER kernel's {WER_MAX_LEN}")
    nflags, nloss = len(state.flag_names), len(state.loss_names)
    if report.numel() != nflags + nloss + 1:
        raise ValueError(f"accumulate: a report of {report.numel()} words does not fit the state's {nflags} flags "
                         f"and {nloss} losses")
    for t in (tokens, lengths, ref, ref_len, report):
        if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous():
            raise RuntimeError("accumulate: contiguous int32 ROCm tensors only.  There is no CPU fallback.")
    counts = torch.empty(G, B, 4, dtype=torch.int32, device=tokens.device)
    L.check(L.lib().sca_eval_accumulate(L.ptr(tokens), L.ptr(lengths), G, B, Hmax, L.ptr(ref), L.ptr(ref_len),
                                        ref.shape[1], L.ptr(report), nflags, nloss, L.ptr(counts), L.ptr(state.state),
                                        L.ptr(state.hyp_log), L.ptr(state.hyp_len_log), state.capacity,
                                        state.log_width, L.stream_handle()), "sca_eval_accumulate")
    return counts


def log_alignments(state, spans, conf, scores):
    """`sca_eval_log_alignments`: one step's alignments (G, B, S, 2) / (G, B, S) / (G, B) appended
    to the state's alignment log at the state's cursor.  Call it BEFORE `accumulate`, which
    advances the cursor."""
    G, B, S = conf.shape
    if G != len(state.keys):
        raise ValueError(f"log_alignments: {G} heads aligned, the state holds {len(state.keys)}")
    if not (spans.is_cuda and spans.dtype == torch.int32 and spans.is_contiguous() and conf.is_cuda and
            conf.dtype == torch.float32 and conf.is_contiguous() and scores.is_cuda and
            scores.dtype == torch.float32 and scores.is_contiguous()):
        raise RuntimeError("log_alignments: contiguous int32 spans and fp32 conf / scores on a ROCm device only.  "
                           "There is no CPU fallback.")
    L.check(L.lib().sca_eval_log_alignments(L.ptr(spans), L.ptr(conf), L.ptr(scores), G, B, S, L.ptr(state.state),
                                            L.ptr(state.span_log), L.ptr(state.conf_log), L.ptr(state.score_log),
                                            state.capacity, state.log_width, L.stream_handle()),
            "sca_eval_log_alignments")


def decode_and_align(outputs, keys, ensembles, beam_size, align, rescoring=None):
    """The tail `eval_step` and `recognize_step` share, on a forward's `outputs` (modified in
    place): the `ensembles` under their keys, the grouped decode of `keys` with
    outputs["input_lengths"] into `tokens` (G, B, T') / `lengths` (G, B) and, with `align`, the
    forced alignment of every decoded tensor's own hypothesis into `spans` (G, B, T', 2), `conf`
    (G, B, T') and `align_scores` (G, B), both fp32.  Returns the decode's scores (G, B), which the
    caller may publish.  No host read.

    `rescoring` (a `Rescoring`, nbest.py): the grouped n-best decode, the rescore and, for
    select="mbr", the MBR selection replace the 1-best decode; `tokens` / `lengths` hold the
    selected hypothesis, the returned scores its total, and `outputs` gains `nbest_tokens`
    (G, B, N, T'), `nbest_lengths`, `nbest_totals`, `nbest_posterior`, `nbest_order` (G, B, N)
    and `nbest_count` (G, B).  None: exactly the calls above, nothing more."""
    add_ensembles(outputs, ensembles)
    logits = [outputs[k] for k in keys]
    if rescoring is not None:
        res = rescored_decode(logits, outputs["input_lengths"], beam_size, rescoring, "decode_and_align")
        tokens, lengths, scores = res.pop("tokens"), res.pop("lengths"), res.pop("scores")
        outputs.update(res)
    else:
        tokens, lengths, scores = ctc_decode_heads_device(logits, outputs["input_lengths"], beam_size)
    outputs["tokens"], outputs["lengths"] = tokens, lengths
    if align:
        res = ctc_align_heads_device(logits, outputs["input_lengths"], tokens, lengths)
        outputs["spans"], outputs["conf"], outputs["align_scores"] = res.spans, res.conf.float(), res.scores.float()
    return scores


def eval_step(model, src_input, state, beam_size=5, rescoring=None):
    """One evaluation step of MSCA_Net, enqueued on the current stream without a host read:
    forward under no_grad with the finite check deferred (a `model.check` of "off" is kept),
    the grouped decode of `state.heads` with outputs["input_lengths"] (`beam_size=0`: greedy),
    and `sca_eval_accumulate` against gloss_labels / gloss_lengths.  Returns the forward's
    outputs plus `tokens` (G, B, T') / `lengths` (G, B) / `counts` (G, B, 4) of this step.

    With `state.align`, every head's own hypothesis is force-aligned to its logits after the
    decode (`sca_ctc_align_heads` with one label set per head) and logged before the
    accumulation: the outputs also hold `spans` (G, B, T', 2), `conf` (G, B, T') and
    `align_scores` (G, B).

    With `state.ensembles`, each ensemble is computed right after the forward (one launch,
    `ensemble_log_probs`), put in the outputs under its key and decoded, aligned, scored and
    logged as one more head after the plain ones: G = len(state.keys).

    With `rescoring` (a `Rescoring`, nbest.py), the n-best decode, the rescore and the selection
    replace the 1-best decode: `tokens` / `lengths` are the selected hypotheses, which are aligned,
    scored and logged as above, and the outputs also hold the `nbest_*` tensors of
    `decode_and_align`.

    The model's `training` flag is left as it is: put the model in `eval()` first."""
    check_rescoring(rescoring, beam_size, "eval_step")
    with torch.no_grad():
        with deferred_check(model):
            outputs = model(src_input)
        if _students_of(outputs) != state.students:
            raise ValueError("eval_step: the model's distillation terms differ from the state's")
        decode_and_align(outputs, state.keys, state.ensembles, beam_size, state.align, rescoring)
        tokens, lengths = outputs["tokens"], outputs["lengths"]
        ref, ref_len = _references(src_input, tokens.shape[1], tokens.device)
        if state.align:
            log_alignments(state, outputs["spans"], outputs["conf"], outputs["align_scores"])
        outputs["counts"] = accumulate(state, tokens, lengths, ref, ref_len, outputs["finite_report"])
    return outputs


# ------------------------------------------------------------------------------- buckets
def _check_wer_limits(buckets, n_pool, label_bucket):
    for f in buckets:
        if f >> n_pool > WER_MAX_LEN:
            raise ValueError(f"BucketedEvalStep: bucket {f} has {f >> n_pool} pooled frames, more than the "
                             f"{WER_MAX_LEN} tokens the WER matrix holds")
    if label_bucket > WER_MAX_LEN:
        raise ValueError(f"BucketedEvalStep: label_bucket {label_bucket} exceeds the {WER_MAX_LEN} tokens the WER "
                         "matrix holds")


def check_eval_buckets(cfg, frame_buckets, label_bucket):
    """Constructor validation of BucketedEvalStep (host only): the sorted bucket tuple."""
    buckets = check_buckets(cfg, frame_buckets, "BucketedEvalStep")
    _check_wer_limits(buckets, n_pool_of(cfg), label_bucket)
    return buckets


class BucketedEvalStep(BucketedStep):
    """`eval_step` for batches of varying length, a subclass of `BucketedStep` (bucketed.py, the
    runner under `BucketedTrainStep`): `step(src_input)` pads the batch to the smallest of
    `frame_buckets` that holds it and to `label_bucket` labels per clip (`pad_batch`,
    `valid_frames`), copies it into the bucket's static device tensors and runs the bucket's
    step, `eval_step`: no optimizer and no hook.  The first use of a bucket runs
    eagerly on a side stream, the second captures the step into a hipGraph (a private pool per
    bucket) and replays it, later uses replay.  A batch whose B differs from `batch_size` runs
    the eager `eval_step` unpadded.  All buckets append to one `EvalState` (`.state`); with
    `capacity` > 0 it logs the hypotheses, `log_width` being the largest bucket's pooled length;
    `align=True` adds the forced alignment of every hypothesis (`alignments()`): a span does not
    depend on the bucket, because the heads' `input_lengths` are the batch's own.  `ensembles`
    are `EvalState`'s: an ensemble row depends on nothing but its frame, so padding changes none.

    Returns the step's outputs, the logits, `tokens` (and `spans`, `conf`) trimmed (views) to the batch's own
    T >> n_pool frames; they are views of the bucket's static outputs, valid until the next
    `step`.  The model must be in `eval()`; a bucket's pooled length and `label_bucket` may not
    exceed 128 (the WER matrix).  `rescoring` is `eval_step`'s; the `nbest_tokens` it adds are
    trimmed like `tokens`."""

    def __init__(self, model, batch_size, frame_buckets, label_bucket, beam_size=5, heads=None, capacity=0,
                 align=False, ensembles=None, rescoring=None):
        super().__init__(model, batch_size, frame_buckets, label_bucket)
        _check_wer_limits(self.frame_buckets, self.n_pool, label_bucket)
        self.beam_size = int(beam_size)
        self.rescoring = check_rescoring(rescoring, self.beam_size, "BucketedEvalStep")
        self.state = EvalState(model, heads, capacity, self.frame_buckets[-1] >> self.n_pool, align, ensembles)

    def read(self):
        return self.state.read()

    def hypotheses(self):
        return self.state.hypotheses()

    def alignments(self, frame_scale=1):
        return self.state.alignments(frame_scale)

    def _device(self):
        return self.state.device

    def _run(self, src):
        return eval_step(self.model, src, self.state, self.beam_size, self.rescoring)

    def _trimmed_keys(self):
        return tuple(self.state.ensembles)
