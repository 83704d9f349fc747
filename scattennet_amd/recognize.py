"""Recognition without references: unlabelled keypoints in, glosses with their frame spans and
confidences out.

* `recognize_step(model, src_input, ...)` — `MSCA_Net.predict` (the label-free forward, finite
  check deferred), the ensembles, the grouped CTC decode and the forced alignment of every
  decoded tensor's own hypothesis, enqueued on the current stream without a host read;
  capturable for a fixed (B, T) by the rules of `train.py`.
* `BucketedRecognizer` — a subclass of `BucketedStep` (bucketed.py) for it: batches of any length
  are padded to a frame bucket, each bucket's step is captured on its second use and replayed
  after.
* `Recognition` — a step's outputs (a dict of device tensors); `read()` is the batch's one host
  read and returns, per clip, {logits_name: [(class id, start, end, confidence), ...]}.
* `rescoring=Rescoring(...)` (nbest.py) on either: the selected hypothesis of every clip's rescored
  n-best list is the one aligned, and `read()` also returns the lists.

The model must be in `eval()` (a model left in training mode recognises with dropout), and the
hypotheses are class ids: the tokenizer stays with the caller.
"""
import numpy as np
import torch

from .align import MAX_LABELS, alignment_lists
from .bucketed import BucketedStep
from .ensemble import check_ensembles
from .evaluate import check_head_keys, decode_and_align, logits_name
from .model import deferred_check, first_error, predict_flag_names
from .nbest import check_rescoring, nbest_lists

_NBEST = ("nbest_count", "nbest_lengths", "nbest_order", "nbest_totals", "nbest_posterior", "nbest_tokens")
_PACKED = ("finite_flags", "lengths", "tokens", "spans", "conf", "align_scores") + _NBEST


class Recognition(dict):
    """The outputs of one recognition step: the logits (the model's five and the ensembles),
    `input_lengths`, `finite_flags`, `tokens` (G, B, T') / `lengths` (G, B) / `scores` (G, B) and,
    with `align`, `spans` (G, B, T', 2), `conf` (G, B, T'), `align_scores` (G, B): device tensors,
    row g belonging to `decoded[g]`.  `frame_scale`: input frames per logit frame."""

    def __init__(self, outputs, decoded, align, frame_scale):
        super().__init__(outputs)
        self.decoded, self.align, self.frame_scale = tuple(decoded), bool(align), int(frame_scale)

    def read(self, frame_scale=None):
        """The batch's one host read, a single packed device-to-host copy.  Raises the
        reference's ValueError (model/__init__.py:130-167) for the first flagged tensor;
        otherwise returns a list of B dicts {logits_name: [(class id, start, end, confidence),
        ...]} (`alignment_lists`: spans in input frames, `frame_scale` defaulting to the
        encoder's 2**n_pool; None for a clip whose hypothesis could not be aligned), or, for a
        step without alignment, {logits_name: [class ids]}.  A step with `rescoring` adds, per
        head, `logits_name + "nbest"`: [(class ids, total, posterior), ...], best total first."""
        scale = self.frame_scale if frame_scale is None else frame_scale
        parts = [self[k] for k in _PACKED if k in self]
        packed = torch.cat([t.reshape(-1).to(torch.float64) for t in parts]).cpu().numpy()  # exact for int32, fp32
        host, at = {}, 0
        for k, t in zip([k for k in _PACKED if k in self], parts):
            host[k] = packed[at:at + t.numel()].reshape(tuple(t.shape))
            at += t.numel()
        msg = first_error(host["finite_flags"].astype(np.int64).tolist(), predict_flag_names())
        if msg is not None:
            raise ValueError(msg)
        tokens, lengths = host["tokens"].astype(np.int64), host["lengths"].astype(np.int64)
        G, B = lengths.shape
        if self.align:
            spans = host["spans"].astype(np.int64)
            per_head = [alignment_lists(tokens[g], lengths[g], spans[g], host["conf"][g], host["align_scores"][g], scale)
                        for g in range(G)]
        else:
            per_head = [[tokens[g, b, :lengths[g, b]].tolist() for b in range(B)] for g in range(G)]
        clips = [{logits_name(k): per_head[g][b] for g, k in enumerate(self.decoded)} for b in range(B)]
        if "nbest_tokens" in host:  # a step with `rescoring`: every list in `order`, from the same copy
            i64 = {k: host[k].astype(np.int64) for k in ("nbest_tokens", "nbest_lengths", "nbest_count", "nbest_order")}
            lists = nbest_lists(i64["nbest_tokens"], i64["nbest_lengths"], host["nbest_totals"], i64["nbest_count"],
                                host["nbest_posterior"], i64["nbest_order"])
            for b in range(B):
                for g, k in enumerate(self.decoded):
                    clips[b][logits_name(k) + "nbest"] = lists[g][b]
        return clips


def _recognize(model, src_input, keys, ensembles, beam_size, align, rescoring=None):
    with torch.no_grad():
        with deferred_check(model):
            outputs = model.predict(src_input)
        decoded = keys + tuple(ensembles)
        outputs["scores"] = decode_and_align(outputs, decoded, ensembles, beam_size, align, rescoring)
    return Recognition(outputs, decoded, align, 2 ** model.n_pool())


def recognize_step(model, src_input, heads=None, ensembles=None, beam_size=5, align=True, rescoring=None):
    """One recognition step of MSCA_Net, enqueued on the current stream without a host read:
    `model.predict(src_input)` under no_grad with the finite check deferred (a `model.check` of
    "off" is kept), the `ensembles` ({output_key: EnsembleSpec}), the grouped decode of `heads`
    (default: the keys evaluate_fn decodes) and the ensembles with `input_lengths`
    (`beam_size=0`: greedy) and, with `align`, the forced alignment of every decoded tensor's own
    hypothesis.  `src_input` needs no label key.  Returns a `Recognition`.  `rescoring` (a
    `Rescoring`, nbest.py): the n-best decode, the rescore and the selection replace the 1-best
    decode; the selected hypothesis is aligned, and `read()` also returns every list.

    The model's `training` flag is left as it is: put the model in `eval()` first."""
    keys = check_head_keys(heads, "recognize_step")
    check_rescoring(rescoring, beam_size, "recognize_step")
    return _recognize(model, src_input, keys, check_ensembles(keys, ensembles, "recognize_step"), int(beam_size),
                      bool(align), rescoring)


class BucketedRecognizer(BucketedStep):
    """`recognize_step` for batches of varying length, a subclass of `BucketedStep` (bucketed.py)
    without labels: `step(src_input)` pads keypoints and mask to the smallest of `frame_buckets`
    that holds the batch (`pad_batch`, `valid_frames`), copies them into the bucket's static
    device tensors and runs the bucket's step.  The first use of a bucket runs eagerly on a side
    stream, the second captures the step into a hipGraph (a private pool per bucket) and replays
    it, later uses replay.  A batch whose B differs from `batch_size` runs the eager step
    unpadded and counts in `eager_fallbacks`.

    `step` returns a `Recognition` with the logits, `tokens`, `spans` and `conf` trimmed (views) to
    the batch's own T >> n_pool frames; they are views of the bucket's static outputs, valid
    until the next `step`.  `Recognition.read()` is the batch's one host read.  The model must be
    in `eval()`; buckets are multiples of 2**n_pool, at most cfg["max_position_embeddings"], and
    with `align` their pooled length may not exceed the alignment's 1023 labels.  `rescoring` is
    `recognize_step`'s."""

    static_keys = ("keypoints", "mask", "valid_len_in", "valid_frames")
    pass_other_keys = False  # nothing else of the batch reaches the step

    def __init__(self, model, batch_size, frame_buckets, beam_size=5, heads=None, ensembles=None, align=True,
                 rescoring=None):
        super().__init__(model, batch_size, frame_buckets)
        if align and self.frame_buckets[-1] >> self.n_pool > MAX_LABELS:
            raise ValueError(f"BucketedRecognizer: bucket {self.frame_buckets[-1]} has "
                             f"{self.frame_buckets[-1] >> self.n_pool} pooled frames, more than the {MAX_LABELS} "
                             "labels the alignment takes")
        self.heads = check_head_keys(heads, "BucketedRecognizer")
        self.ensembles = check_ensembles(self.heads, ensembles, "BucketedRecognizer")
        self.beam_size, self.align = int(beam_size), bool(align)
        self.rescoring = check_rescoring(rescoring, self.beam_size, "BucketedRecognizer",
                                         frames=self.frame_buckets[-1] >> self.n_pool)
        self.device = next(model.parameters()).device

    def _device(self):
        return self.device

    def _run(self, src):
        return _recognize(self.model, src, self.heads, self.ensembles, self.beam_size, self.align, self.rescoring)

    def _trimmed_keys(self):
        return tuple(self.ensembles)

    def _keep(self, rec):
        return Recognition(rec, rec.decoded, rec.align, rec.frame_scale)
