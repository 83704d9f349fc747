"""Minimum word error rate (MWER) training on the device: the expected number of errors of the
n-best hypotheses of a clip under the model's own posterior over that list — exact CTC
likelihoods, error counts from the project's WER alignment — as a differentiable loss
(`sca_mwer_fwd` / `sca_mwer_bwd`; the semantics are the header's, include/scatten.h).  The
reference has none of this.

* `MWERLossOp` — the autograd Function over fp32 logits (B, T, C) and int32 device tensors.
* `mwer_loss` — the validated entry point: decodes the detached logits into an uncollapsed
  n-best list (`ctc_decode_nbest_device`) unless the caller hands one over.
* `MWER` — the validated spec that `train_step(..., mwer=)` and `BucketedTrainStep(..., mwer=)`
  take; `mwer_guard` is the scalar they hand to `FusedAdam.step`.

No call reads the device or allocates outside the caching allocator: everything is usable under
`torch.cuda.graph` capture.
"""
import torch
from torch.autograd import Function

from . import _lib as L
from .decode import MAX_BEAM, WER_MAX_LEN, _check_lengths, _check_logits, check_on_device
from .heads import _dev_i32
from .model import _LOGITS
from .nbest import MAX_CLASSES, _check_beam, _check_nbest, _finite, ctc_decode_nbest_device


class MWERLossOp(Function):
    """(loss, loglik, posterior, errors, risk) of `sca_mwer_fwd` on batch-major fp32 logits
    (B, T, C); in_len (B), tokens (B, N, H), out_len (B, N), count (B), ref (B, R), ref_len (B)
    int32 device tensors.  Only `loss` is differentiable; the workspace (row statistics, alpha,
    beta, the gradient weights) is kept for the backward."""

    @staticmethod
    def forward(ctx, logits, in_len, tokens, out_len, count, ref, ref_len, posterior_scale):
        x = logits.contiguous()
        L.require_device(x)
        B, T, C = x.shape
        N, H = tokens.shape[1], tokens.shape[2]
        lib = L.lib()
        ws = x.new_empty(max(lib.sca_mwer_workspace_floats(B, N, T, H), 1))
        loss = x.new_empty(())
        loglik, posterior = x.new_empty(B, N), x.new_empty(B, N)
        errors = torch.empty(B, N, dtype=torch.int32, device=x.device)
        risk = x.new_empty(B)
        L.check(lib.sca_mwer_fwd(L.ptr(x), L.ptr(in_len), L.ptr(tokens), L.ptr(out_len), L.ptr(count), L.ptr(ref),
                                 L.ptr(ref_len), B, N, T, C, H, ref.shape[1], posterior_scale, L.ptr(loglik),
                                 L.ptr(posterior), L.ptr(errors), L.ptr(risk), L.ptr(loss), L.ptr(ws),
                                 L.stream_handle()), "sca_mwer_fwd")
        ctx.save_for_backward(x, in_len, tokens, out_len, count, ws)
        ctx.mark_non_differentiable(loglik, posterior, errors, risk)
        return loss, loglik, posterior, errors, risk

    @staticmethod
    def backward(ctx, dloss, *_):
        x, in_len, tokens, out_len, count, ws = ctx.saved_tensors
        B, T, C = x.shape
        dloss = dloss.contiguous() if dloss is not None else x.new_zeros(())
        dx = torch.empty_like(x)
        L.check(L.lib().sca_mwer_bwd(L.ptr(x), L.ptr(in_len), L.ptr(tokens), L.ptr(out_len), L.ptr(count), B,
                                     tokens.shape[1], T, C, tokens.shape[2], L.ptr(dloss), L.ptr(ws), L.ptr(dx),
                                     L.stream_handle()), "sca_mwer_bwd")
        return dx, None, None, None, None, None, None, None


def _check_refs(labels, lengths, B, C, what):
    """`heads._validate_ctc`'s checks for the references, with an empty reference allowed; values
    are checked only where that needs no device read (host tensors)."""
    if labels.dim() != 2 or labels.shape[0] != B:
        raise RuntimeError(f"{what}: gloss_labels must be (B, R) padded with B = {B}, got {tuple(labels.shape)}")
    if not 1 <= labels.shape[1] <= WER_MAX_LEN:
        raise ValueError(f"{what}: references of up to {labels.shape[1]} tokens are outside the WER kernel's "
                         f"[1, {WER_MAX_LEN}]")
    if torch.as_tensor(lengths).numel() != B:
        raise RuntimeError(f"Expected gloss_lengths to have {B} entries (one per clip), got "
                           f"{torch.as_tensor(lengths).numel()}")
    rl = torch.as_tensor(lengths)
    if rl.device.type == "cpu" and B:  # device lengths are trusted: the kernels clamp them, no host read
        if int(rl.max()) > labels.shape[1] or int(rl.min()) < 0:
            raise RuntimeError(f"{what}: gloss_lengths must lie in [0, {labels.shape[1]}], got "
                               f"[{int(rl.min())}, {int(rl.max())}]")
    if labels.device.type == "cpu" and labels.numel():
        lo, hi = int(labels.min()), int(labels.max())
        if lo < 0 or hi >= C:
            raise RuntimeError(f"target values must lie in [0, {C}); got [{lo}, {hi}]")


def mwer_loss(gloss_logits, input_lengths, gloss_labels, gloss_lengths, nbest=None, beam_size=5, nbest_size=None,
              posterior_scale=1.0, return_details=False):
    """The MWER loss (0-dim, differentiable with respect to `gloss_logits`) of batch-major logits
    (B, T, C) against the references `gloss_labels` (B, R) padded / `gloss_lengths` (B); a
    reference may be empty.  `nbest=None`: the list is the `nbest_size` (default `beam_size`) best
    labellings of `ctc_decode_nbest_device(..., collapse_repeats=False)` on the detached logits —
    uncollapsed lists hold distinct labellings, which is what a posterior needs.  Otherwise
    `nbest` is an `NBest` (tokens (B, N, H), lengths (B, N), scores — not read —, count (B)) on
    the logits' device.  With `return_details` also a dict of device tensors: `loglik` (B, N) (the
    exact CTC log-likelihoods, -inf for entries that do not exist or do not fit), `posterior`
    (B, N), `errors` (B, N) int32, `risk` (B).  T, H and R are limited by the WER kernel's 128
    tokens.  No host sync under capture; capturable."""
    what = "mwer_loss"
    _check_logits(gloss_logits)
    B, T, C = gloss_logits.shape
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"{what}: logits of {C} classes are outside [1, {MAX_CLASSES}]")
    ps = _finite("posterior_scale", posterior_scale, what)
    il = _check_lengths(input_lengths, B, T)
    labels = torch.as_tensor(gloss_labels)
    _check_refs(labels, gloss_lengths, B, C, what)
    if nbest is None:
        beam, n = _check_beam(beam_size, nbest_size)
        if T > WER_MAX_LEN:
            raise ValueError(f"{what}: hypotheses over {T} logit frames exceed the WER kernel's {WER_MAX_LEN} tokens")
    else:
        G, Bn, _, H = _check_nbest(nbest, what)
        if nbest.tokens.dim() != 3 or Bn != B:
            raise RuntimeError(f"{what}: the list must be a single head's, tokens (B = {B}, N, H), got "
                               f"{tuple(nbest.tokens.shape)}")
        if H > WER_MAX_LEN:
            raise ValueError(f"{what}: hypotheses of up to {H} tokens exceed the WER kernel's {WER_MAX_LEN}")
    check_on_device(None, gloss_logits)
    dev = gloss_logits.device
    in_len = _dev_i32(il, dev)
    if nbest is None:
        nbest = ctc_decode_nbest_device(gloss_logits, in_len, beam, n, collapse_repeats=False)
    else:
        check_on_device(what, nbest.tokens, nbest.lengths, nbest.count)
    x = gloss_logits if gloss_logits.dtype == torch.float32 else gloss_logits.float()
    loss, loglik, posterior, errors, risk = MWERLossOp.apply(
        x, in_len, _dev_i32(nbest.tokens, dev), _dev_i32(nbest.lengths, dev), _dev_i32(nbest.count, dev),
        _dev_i32(labels, dev), _dev_i32(torch.as_tensor(gloss_lengths).reshape(-1), dev), ps)
    if return_details:
        return loss, {"loglik": loglik, "posterior": posterior, "errors": errors, "risk": risk}
    return loss


class MWER:
    """What `train_step` and `BucketedTrainStep` add to the step as `mwer=`: the MWER loss of the
    logits `head` (one of the model's five), with the list decoded per step by a beam of
    `beam_size` (1 <= beam_size <= 32) keeping `nbest` entries (default: all of the beam), the
    posterior sharpened by `posterior_scale`, and `weight` (finite, >= 0) times the loss added to
    `total_loss` for the backward.  ValueError for anything else."""

    def __init__(self, weight, beam_size=5, nbest=None, posterior_scale=1.0, head="fuse_coord_gloss_logits"):
        for v in (weight, posterior_scale):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise ValueError(f"MWER: weight and posterior_scale must be numbers, got {v!r}")
        self.weight = _finite("weight", weight, "MWER")
        self.posterior_scale = _finite("posterior_scale", posterior_scale, "MWER")
        if self.weight < 0.0:
            raise ValueError(f"MWER: weight must not be negative, got {weight!r}")
        for name, v in (("beam_size", beam_size), ("nbest", nbest)):
            if v is None and name == "nbest":
                continue
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_BEAM:
                raise ValueError(f"MWER: {name} must be an int in [1, {MAX_BEAM}], got {v!r}")
        if nbest is not None and nbest > beam_size:
            raise ValueError(f"MWER: nbest = {nbest} exceeds beam_size = {beam_size}")
        if head not in _LOGITS:
            raise ValueError(f"MWER: head must be one of {_LOGITS}, got {head!r}")
        self.beam_size, self.nbest, self.head = beam_size, beam_size if nbest is None else nbest, head

    def __repr__(self):
        return (f"MWER(weight={self.weight}, beam_size={self.beam_size}, nbest={self.nbest}, posterior_scale="
                f"{self.posterior_scale}, head={self.head!r})")


def check_mwer(mwer, what):
    """`mwer=` of a step, validated on the host: None or an `MWER`."""
    if mwer is not None and not isinstance(mwer, MWER):
        raise ValueError(f"{what}: mwer must be an MWER or None, got {type(mwer).__name__}")
    return mwer


def mwer_guard(guard, mwer_loss_value):
    """The scalar a step with MWER hands to `FusedAdam.step`: `guard` when `mwer_loss_value` is
    finite, NaN otherwise (the update is then skipped on the device).  0-dim device tensors; no
    host read."""
    return guard + mwer_loss_value.detach().to(guard.dtype) * 0.0  # inf * 0 = nan * 0 = nan
