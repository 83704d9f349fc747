"""Length-bucketed training step: one captured hipGraph per frame bucket.

A captured `train_step` holds for one fixed (B, T, S), but a training collator draws a new
length per clip (`select_frames`), so T changes with almost every batch.  Here a batch of any
T <= T_bucket is zero-padded to the bucket (`pad_batch`) and run through that bucket's graph.
`valid_frames`, a device scalar holding the batch's own T, keeps the three ops through which
the added frames would reach the valid ones (fusion softmax, SeqKD, the BiLSTM's reverse
direction) to the valid frames; the losses, the valid frames' logits and every parameter
gradient are then those of the unpadded batch.

Dropout: the counter-based masks are indexed by position in the padded tensor, so a training-
mode bucketed run draws different (equally valid) masks than the unpadded run of the same batch.
Data parallelism (`dp.py`) is not wired to this step.
"""
import bisect

import torch

from . import heads
from .encoder import n_pool_of
from .model import _LOGITS
from .distill import check_distill
from .mwer import check_mwer
from .train import step_parameters, train_step


def pad_batch(src_input, frames, labels=None):
    """A copy of `src_input` zero-padded to a bucket: keypoints (B, frames, K, 2), mask
    (B, frames), and — with `labels` — gloss_labels (B, labels) (2-D labels padded with 0; 1-D
    concatenated labels split by gloss_lengths first).  The length tensors stay as they are.
    Adds `valid_frames` = [T] (int32, on the keypoints' device): the batch's own length, which
    MSCA_Net hands to the ops that must not see the added frames.  Pure torch, host or device
    tensors; the input dict is not modified.  ValueError when frames < T or labels < S."""
    kp, mask = src_input["keypoints"], src_input["mask"]
    B, T = kp.shape[0], kp.shape[1]
    if mask.shape[0] != B or mask.shape[1] != T:
        raise ValueError(f"pad_batch: mask {tuple(mask.shape)} does not match keypoints {tuple(kp.shape)}")
    if frames < T:
        raise ValueError(f"pad_batch: the batch has {T} frames, more than the bucket's {frames}")
    out = dict(src_input)
    pk = kp.new_zeros((B, frames) + tuple(kp.shape[2:]))
    pk[:, :T] = kp
    pm = mask.new_zeros(B, frames)
    pm[:, :T] = mask
    out["keypoints"], out["mask"] = pk, pm
    if labels is not None:
        lab = heads.labels_2d(src_input, B, "pad_batch")
        if labels < lab.shape[1]:
            raise ValueError(f"pad_batch: the batch has {lab.shape[1]} labels per clip, more than the "
                             f"bucket's {labels}")
        pl = lab.new_zeros(B, labels)
        pl[:, :lab.shape[1]] = lab
        out["gloss_labels"] = pl
    out["valid_frames"] = torch.tensor([T], dtype=torch.int32, device=kp.device)
    return out



def pick_bucket(frame_buckets, T, who="pick_bucket"):
    """The smallest bucket >= T of the sorted `frame_buckets`; ValueError (under the caller's
    name `who`) when none fits."""
    i = bisect.bisect_left(frame_buckets, T)
    if i == len(frame_buckets):
        raise ValueError(f"{who}: a batch of {T} frames fits no bucket (largest: {frame_buckets[-1]})")
    return frame_buckets[i]


def check_buckets(cfg, frame_buckets, who):
    """Constructor validation of a bucketed step (host only): the sorted bucket tuple.  `who`,
    the caller's class name, opens every message."""
    buckets = tuple(sorted(int(f) for f in frame_buckets))
    if not buckets or len(set(buckets)) != len(buckets):
        raise ValueError(f"{who}: frame_buckets must be distinct and non-empty, got {frame_buckets!r}")
    step = 2 ** n_pool_of(cfg)
    for f in buckets:
        if f < step or f % step:
            raise ValueError(f"{who}: bucket {f} is not a multiple of 2**n_pool = {step} (the pooled "
                             "length of a bucket must not depend on rounding)")
        if f > cfg["max_position_embeddings"]:
            raise ValueError(f"{who}: bucket {f} exceeds max_position_embeddings = "
                             f"{cfg['max_position_embeddings']}")
    return buckets


class _Bucket:
    def __init__(self, frames):
        self.frames = frames
        self.static = None    # the device tensors every run of this bucket reads
        self.graph = None
        self.outputs = None   # the captured step's outputs: replays refill them
        self.pool = None
        self.uses = 0


class BucketedStep:
    """The runner under `BucketedTrainStep`, `BucketedEvalStep` and `BucketedRecognizer`, and the
    one place that follows the capture rules of DESIGN.md §5d: `step(src_input)` pads the batch
    to the smallest of `frame_buckets` that holds it (`pad_batch`, with `label_bucket` labels per
    clip unless that is None), copies the `static_keys` into the bucket's static device tensors
    and runs the bucket's step.  The first use of a bucket runs `_run` eagerly on a side stream,
    the second captures it into a hipGraph (a private pool per bucket) and replays it, every
    later use replays.  A batch whose B differs from `batch_size` runs `_run` eagerly, unpadded,
    and counts in `eager_fallbacks`.  Every return is `_keep`'s copy of the outputs with the
    logits, `tokens`, `spans` and `conf` trimmed (views) to the batch's own T >> n_pool frames.

    A subclass sets `static_keys`, defines `_device()` and `_run(src)`, and may override
    `pass_other_keys` (False: the step sees the static tensors only), `_trimmed_keys()` (logit
    keys beside the model's five), `_keep(outputs)` (default: a plain dict copy) and the two
    hooks `_before_replay()` and `_before_capture()`.  The constructor validates on the host
    and touches no tensor of the model; messages carry the subclass's name."""

    static_keys = ("keypoints", "mask", "valid_len_in", "gloss_labels", "gloss_lengths", "valid_frames")
    pass_other_keys = True  # the batch's other keys reach `_run` beside the static tensors

    def __init__(self, model, batch_size, frame_buckets, label_bucket=None):
        who = type(self).__name__
        self.frame_buckets = check_buckets(model.cfg, frame_buckets, who)
        if batch_size < 1 or (label_bucket is not None and label_bucket < 1):
            raise ValueError(f"{who}: batch_size{'' if label_bucket is None else ' and label_bucket'} must be positive")
        self.model, self.batch_size = model, int(batch_size)
        self.label_bucket = None if label_bucket is None else int(label_bucket)
        self.n_pool = n_pool_of(model.cfg)
        self._buckets = {f: _Bucket(f) for f in self.frame_buckets}
        self._stream = None
        self.eager_fallbacks = 0

    @property
    def graphs_captured(self):
        return sum(b.graph is not None for b in self._buckets.values())

    def captured(self, frames):
        """Whether the bucket of `frames` frames (one of `frame_buckets`) holds its graph."""
        return self._buckets[frames].graph is not None

    def bucket_for(self, T):
        return pick_bucket(self.frame_buckets, T, type(self).__name__)

    # ------------------------------------------------------------ what a subclass supplies
    def _device(self):
        raise NotImplementedError

    def _run(self, src):
        """The step itself, enqueued on the current stream without a host read."""
        raise NotImplementedError

    def _trimmed_keys(self):
        return ()

    def _keep(self, outputs):
        return dict(outputs)

    def _before_replay(self):
        """Runs before a pure replay (not before the replay that follows a capture)."""

    def _before_capture(self):
        """Runs on a bucket's second use, before the device synchronise and the capture."""

    # ------------------------------------------------------------------------- the protocol
    def _fill(self, bucket, padded, device):
        keys = self.static_keys
        if bucket.static is None:
            bucket.static = {}
            for k in keys:
                t = torch.as_tensor(padded[k])
                bucket.static[k] = torch.empty(t.shape, dtype=t.dtype, device=device)
        for k in keys:
            t = torch.as_tensor(padded[k])
            if t.shape != bucket.static[k].shape or t.dtype != bucket.static[k].dtype:
                raise ValueError(f"{type(self).__name__}: {k} changed from {tuple(bucket.static[k].shape)} "
                                 f"{bucket.static[k].dtype} to {tuple(t.shape)} {t.dtype} between batches")
            bucket.static[k].copy_(t, non_blocking=True)
        if not self.pass_other_keys:
            return dict(bucket.static)
        extra = {k: v for k, v in padded.items() if k not in keys}
        return {**extra, **bucket.static}

    def _trim(self, outputs, T):
        n = T >> self.n_pool
        out = self._keep(outputs)
        for k in _LOGITS + self._trimmed_keys():
            if k in out:
                out[k] = out[k][:, :n]
        for k in ("tokens", "spans", "conf"):
            if k in out:
                out[k] = out[k][:, :, :n]
        if "nbest_tokens" in out:  # (G, B, N, T')
            out["nbest_tokens"] = out["nbest_tokens"][..., :n]
        return out

    def step(self, src_input):
        kp = src_input["keypoints"]
        B, T = kp.shape[0], kp.shape[1]
        if B != self.batch_size:
            self.eager_fallbacks += 1
            # kept (`_keep`) like every other step's outputs: an autograd graph of this model that
            # is still alive when a bucket is captured hands the captured backward its gradient
            # accumulators, which belong to the stream THIS step ran on
            return self._trim(self._run(src_input), T)
        bucket = self._buckets[self.bucket_for(T)]
        device = self._device()
        src = self._fill(bucket, pad_batch(src_input, bucket.frames, self.label_bucket), device)
        bucket.uses += 1
        if bucket.graph is not None:
            self._before_replay()
            bucket.graph.replay()
            return self._trim(bucket.outputs, T)
        if bucket.uses == 1:  # warm-up: a real eager step, on a side stream as capture will be
            if self._stream is None:
                self._stream = torch.cuda.Stream(device=device)
            self._stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._stream):
                outputs = self._run(src)
            torch.cuda.current_stream().wait_stream(self._stream)
            return self._trim(outputs, T)
        # second use: capture, then the replay is this batch's step
        self._before_capture()
        torch.cuda.synchronize()
        bucket.pool = torch.cuda.graph_pool_handle()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, pool=bucket.pool):
            outputs = self._run(src)
        bucket.outputs = self._keep(outputs)
        del outputs
        bucket.graph = graph
        graph.replay()
        return self._trim(bucket.outputs, T)


class BucketedTrainStep(BucketedStep):
    """`train_step` for batches of varying length: `step(src_input)` pads the batch to the
    smallest of `frame_buckets` that holds it and to `label_bucket` labels per clip, copies it
    into that bucket's static device tensors and runs the bucket's step.

    The first use of a bucket is an eager `train_step` on a side stream (a real step; it also
    lets the optimizer and the library allocate their lazy state), the second use captures
    the step into a hipGraph and replays it, every later use replays.  A batch whose B differs
    from `batch_size` (an epoch's last batch) runs the plain eager `train_step` unpadded.

    Returns the step's outputs with the logits trimmed (views) to the batch's own
    T >> n_pool frames; `read_report` works on them as on `train_step`'s.  They are views of
    the bucket's static outputs: valid until the next `step` (of any bucket: copy what must
    outlive it).  Every step hands out detached tensors, so nothing it returns keeps an
    autograd graph alive; a caller that runs this model outside `step` must drop those outputs
    before a bucket's second use (capture rules: a captured backward must not
    find an earlier step's autograd graph alive).

    Buckets must be multiples of 2**n_pool and at most cfg["max_position_embeddings"]; the
    optimizer needs `capture_slots >= len(frame_buckets)`.  `label_bucket` is the largest
    label count per clip (at most the CTC kernels' limit).  `step` uploads the optimizer's
    hyper-parameters before a replay when a scheduler changed them.  `mwer`: None or an `MWER`,
    handed to `train_step`; the added frames lie past `input_lengths`, so the MWER loss and its
    gradients are those of the unpadded batch; that holds for every form of the spec (several
    heads, the reference as an entry, the gloss model's prior, the fused search): the padded
    labels lie past `gloss_lengths` as the frames lie past `input_lengths`.  `distill`: None or a
    `Distill`, handed to `train_step`, which passes the bucket's `valid_frames` to the grouped
    call: the added frames contribute exact zeros, so the term and its gradients are the
    unpadded batch's.

    Memory: every bucket keeps its own graph memory pool — all activations, gradients and
    workspaces of one step at (batch_size, bucket) stay reserved for the graph's lifetime, so
    the cost is about the sum over buckets of an eager step's peak at that length (parameters
    and optimizer state are shared, not duplicated)."""

    def __init__(self, model, optimizer, batch_size, frame_buckets, label_bucket, mwer=None, distill=None):
        super().__init__(model, batch_size, frame_buckets, label_bucket)
        self.mwer = check_mwer(mwer, "BucketedTrainStep")
        self.distill = check_distill(distill, "BucketedTrainStep")
        n, slots = len(self.frame_buckets), getattr(optimizer, "capture_slots", 0)
        if slots < n:
            raise ValueError(f"BucketedTrainStep: {n} buckets need an optimizer with capture_slots >= {n} (one "
                             f"captured step each), got {slots}: FusedAdam(..., capture_slots={n})")
        self.optimizer = optimizer

    def _device(self):  # looked up per step: the constructor touches no tensor of the model
        return next(self.model.parameters()).device

    def _run(self, src):
        kw = {} if self.distill is None else {"distill": self.distill}
        if self.mwer is None:
            return train_step(self.model, self.optimizer, src, **kw)
        return train_step(self.model, self.optimizer, src, mwer=self.mwer, **kw)

    def _keep(self, outputs):
        """Detached: the step's backward has run, and an autograd graph a caller keeps alive must
        not be around when a later step is captured."""
        return {k: v.detach() if torch.is_tensor(v) else v for k, v in outputs.items()}

    def _before_replay(self):  # a scheduler may have stepped since the last upload
        if self.optimizer.hyperparameters_changed():
            self.optimizer.sync_hyperparameters()

    def _before_capture(self):
        # No autograd graph of an earlier step is alive (every step handed out detached outputs
        # only) and the group table is current; the gradients of the last step are dropped so
        # that the graph's own live in its pool (a LearnedEnsemble head's among them).
        for p in step_parameters(self.model, self.mwer):
            p.grad = None
        self._before_replay()  # the captured step reads the same hyper-parameter table
