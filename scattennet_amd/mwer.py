"""Minimum word error rate (MWER) training on the device: the expected number of errors of the
n-best hypotheses of a clip under the model's own posterior over that list — exact CTC
likelihoods, error counts from the project's WER alignment — as a differentiable loss
(`sca_mwer_heads_fwd` / `sca_mwer_heads_bwd`; the semantics are the header's, include/scatten.h).
The reference has none of this.

* `MWERLossOp` — the one autograd Function: fp32 logits (B, T, C) of G heads in one call and int32
  device tensors, optionally with each clip's reference as one more entry of its list and with
  the bigram gloss model's prior inside the posterior.  A single tensor is its G = 1 call.
* `mwer_loss` — the validated entry point, for one tensor or a sequence of them: decodes the
  detached logits into an uncollapsed n-best list (the plain search, or the fused one) unless
  the caller hands one over.
* `MWER` — the validated spec that `train_step(..., mwer=)` and `BucketedTrainStep(..., mwer=)`
  take; `mwer_guard` is the scalar they hand to `FusedAdam.step`.

No call reads the device or allocates outside the caching allocator: everything is usable under
`torch.cuda.graph` capture.
"""
import ctypes

import torch
from torch.autograd import Function

from . import _lib as L
from .ensemble import EnsembleSpec, LearnedEnsemble
from .decode import MAX_BEAM, WER_MAX_LEN, _check_lengths, _check_logits, check_heads, check_on_device
from .heads import _dev_i32
from .model import _LOGITS
from .nbest import (MAX_CLASSES, MAX_HEADS, BigramLM, _check_beam, _check_fusion, _check_nbest, _dense_only,
                    _finite, _fusion_table, _nbest_decode)
from .ngram import NGramLM


class MWERLossOp(Function):
    """(loss (G), loglik, posterior, errors (G, B, M), ref_valid (G, B), risk (G, B)) of
    `sca_mwer_heads_fwd` on the G batch-major fp32 logits `*logits`, each (B, T, C); with
    `grouped=False` (one tensor) the results have no head axis and `loss` is 0-dim, so that the
    caller's backward needs no indexing kernels; in_len (B),
    tokens (G, B, N, H), out_len (G, B, N), count (G, B), ref (B, R), ref_len (B) int32 device
    tensors; `with_ref`: the reference is slot N of every list (M = N + 1, else M = N); `table`:
    the (C, C) fp32 device table of the prior, an `NGramLM` on the device (`sca_mwer_heads_fwd_ngram`;
    the backward is the same) or None, with `lm_weight` and `length_bonus`.
    Only `loss` is differentiable, with respect to every head's logits; the workspace is kept for
    the backward."""

    @staticmethod
    def forward(ctx, in_len, tokens, out_len, count, ref, ref_len, posterior_scale, with_ref, table, lm_weight,
                length_bonus, grouped, *logits):
        xs = [x.contiguous() for x in logits]
        sparse = isinstance(table, NGramLM)
        L.require_device(*xs, table.uni_lp if sparse else table)
        G = len(xs)
        B, T, C = xs[0].shape
        N, H = tokens.shape[-2], tokens.shape[-1]
        R, M = ref.shape[1], N + int(with_ref)
        lib, x = L.lib(), xs[0]
        ws = x.new_empty(max(lib.sca_mwer_heads_workspace_floats(G, B, N, T, H, R, int(with_ref)), 1))
        if not grouped and G != 1:
            raise RuntimeError("MWERLossOp: grouped=False takes one logits tensor")
        lead = (G, B) if grouped else (B,)
        loss = x.new_empty(lead[:-1])
        loglik, posterior = x.new_empty(lead + (M,)), x.new_empty(lead + (M,))
        errors = torch.empty(lead + (M,), dtype=torch.int32, device=x.device)
        ref_valid = torch.empty(lead, dtype=torch.int32, device=x.device)
        risk = x.new_empty(lead)
        hx = L.decode_heads(xs)
        fwd, name = (lib.sca_mwer_heads_fwd_ngram, "sca_mwer_heads_fwd_ngram") if sparse else \
            (lib.sca_mwer_heads_fwd, "sca_mwer_heads_fwd")
        L.check(fwd(ctypes.byref(hx), G, L.ptr(in_len), L.ptr(tokens), L.ptr(out_len), L.ptr(count), L.ptr(ref),
                    L.ptr(ref_len), B, N, T, C, H, R, int(with_ref),
                    ctypes.byref(table.struct) if sparse else L.ptr(table), lm_weight, length_bonus, posterior_scale, L.ptr(loglik), L.ptr(posterior), L.ptr(errors),
                    L.ptr(ref_valid), L.ptr(risk), L.ptr(loss), L.ptr(ws), L.stream_handle()), name)
        ctx.lm = table if sparse else None  # the trie's tensors stay alive with the graph of this call
        ctx.save_for_backward(in_len, tokens, out_len, count, ref, ref_len, ws, *xs)
        ctx.with_ref = int(with_ref)
        ctx.mark_non_differentiable(loglik, posterior, errors, ref_valid, risk)
        # the backward reads dloss alone: without this autograd fills one zero tensor per detail
        # first, five small launches in every backward
        ctx.set_materialize_grads(False)
        return loss, loglik, posterior, errors, ref_valid, risk

    @staticmethod
    def backward(ctx, dloss, *_):
        in_len, tokens, out_len, count, ref, ref_len, ws, *xs = ctx.saved_tensors
        G = len(xs)
        B, T, C = xs[0].shape
        dloss = dloss.contiguous() if dloss is not None else xs[0].new_zeros(G)
        dxs = [torch.empty_like(x) for x in xs]
        hx, gx = L.decode_heads(xs), L.MwerGrads()
        for g, dx in enumerate(dxs):
            gx.dlogits[g] = dx.data_ptr()
        L.check(L.lib().sca_mwer_heads_bwd(ctypes.byref(hx), G, L.ptr(in_len), L.ptr(tokens), L.ptr(out_len),
                                           L.ptr(count), L.ptr(ref), L.ptr(ref_len), B, tokens.shape[-2], T, C,
                                           tokens.shape[-1], ref.shape[1], ctx.with_ref, L.ptr(dloss), L.ptr(ws),
                                           ctypes.byref(gx), L.stream_handle()), "sca_mwer_heads_bwd")
        return (None,) * 12 + tuple(dxs)


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


def _check_prior(lm, lm_weight, length_bonus, fusion, num_classes, what):
    """The prior's arguments, validated on the host: (lm as a BigramLM, an NGramLM or None,
    lm_weight, length_bonus).  `lm` may also be a (C, C) table of finite log-probabilities (a
    device table is then read once: hand over a `BigramLM` under capture)."""
    if fusion is True:
        _dense_only(lm, what)
    if lm is not None and not isinstance(lm, (BigramLM, NGramLM)):
        if not (torch.is_tensor(lm) or hasattr(lm, "__array__")):
            raise ValueError(f"{what}: lm must be a BigramLM, an NGramLM, a (C, C) table or None, got "
                             f"{type(lm).__name__}")
        lm = BigramLM(lm)
    try:
        if num_classes is None and lm is not None:
            num_classes = lm.num_classes
        lw, lb = _check_fusion(lm, lm_weight, length_bonus, num_classes, what)
    except TypeError:
        raise ValueError(f"{what}: lm_weight and length_bonus must be numbers") from None
    if not isinstance(fusion, bool):
        raise ValueError(f"{what}: fusion must be a bool, got {fusion!r}")
    if fusion and lm is None and lb == 0.0:
        raise ValueError(f"{what}: fusion=True needs a gloss model or a length bonus: there is nothing to fuse")
    return lm, lw, lb


def mwer_loss(gloss_logits, input_lengths, gloss_labels, gloss_lengths, nbest=None, beam_size=5, nbest_size=None,
              posterior_scale=1.0, return_details=False, *, reference=False, lm=None, lm_weight=0.0,
              length_bonus=0.0, fusion=False):
    """The MWER loss (0-dim, differentiable with respect to `gloss_logits`) of batch-major logits
    (B, T, C) against the references `gloss_labels` (B, R) padded / `gloss_lengths` (B); a
    reference may be empty.  `nbest=None`: the list is the `nbest_size` (default `beam_size`) best
    labellings of `ctc_decode_nbest_device(..., collapse_repeats=False)` on the detached logits —
    uncollapsed lists hold distinct labellings, which is what a posterior needs.  Otherwise
    `nbest` is an `NBest` (tokens (B, N, H), lengths (B, N), scores — not read —, count (B)) on
    the logits' device.  With `return_details` also a dict of device tensors: `loglik` (B, N) (the
    exact CTC log-likelihoods, -inf for entries that do not exist or do not fit), `posterior`
    (B, N), `errors` (B, N) int32, `risk` (B).  T, H and R are limited by the WER kernel's 128
    tokens.  No host sync under capture; capturable.

    Keyword-only, all off by default (the call is then exactly the above):
    `reference=True` makes each clip's reference one more entry of its list, slot N of N + 1 (the
    details' last axis): error count 0, its own exact likelihood, left out of the posterior where
    the list holds the reference already or the reference does not fit in `input_lengths` frames;
    `ref_valid` (B) int32 in the details says where it counts, and `loglik[:, N]` is the
    reference's likelihood wherever it fits.  A list whose hypotheses are all equally wrong then
    has a gradient, towards the transcript.
    `lm` (a `BigramLM` or an `NGramLM` on the logits' device, or a (C, C) table), `lm_weight`, `length_bonus`: the
    posterior is the softmax of posterior_scale * (ll + lm_weight * lm(h) + length_bonus * len(h)),
    the total `rescore_nbest_device` ranks by, for the reference slot too.
    `fusion=True` (with `nbest=None`) takes the list from `ctc_decode_fused_nbest_device(...,
    collapse_repeats=False)` with the same table and weights.
    `gloss_logits` may be a sequence of G tensors of one shape, the heads of one forward, with the
    references shared: the lists are decoded by the grouped decoders, or `nbest` is a heads-form
    `NBest` (tokens (G, B, N, H)); one grouped call then returns `loss` (G), one mean per head,
    and details with a leading G axis, `ref_valid` (G, B) among them.  Head g is bitwise the
    single-tensor call on it."""
    what = "mwer_loss"
    grouped = isinstance(gloss_logits, (list, tuple))
    if grouped:
        xs = check_heads(gloss_logits, what)
    else:
        _check_logits(gloss_logits)
        xs = [gloss_logits]
    G = len(xs)
    B, T, C = xs[0].shape
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError(f"{what}: logits of {C} classes are outside [1, {MAX_CLASSES}]")
    if G * B > 65535:
        raise ValueError(f"{what}: {G} heads of {B} clips exceed the 65535 (head, clip) pairs of one call")
    if not isinstance(reference, bool):
        raise ValueError(f"{what}: reference must be a bool, got {reference!r}")
    ps = _finite("posterior_scale", posterior_scale, what)
    lm, lw, lb = _check_prior(lm, lm_weight, length_bonus, fusion, C, what)
    il = _check_lengths(input_lengths, B, T)
    labels = torch.as_tensor(gloss_labels)
    _check_refs(labels, gloss_lengths, B, C, what)
    if nbest is None:
        beam, n = _check_beam(beam_size, nbest_size)
        if T > WER_MAX_LEN:
            raise ValueError(f"{what}: hypotheses over {T} logit frames exceed the WER kernel's {WER_MAX_LEN} tokens")
    else:
        if fusion:
            raise ValueError(f"{what}: fusion=True decodes the list itself; it does not go with nbest=")
        Gn, Bn, _, H = _check_nbest(nbest, what)
        if nbest.tokens.dim() != (4 if grouped else 3) or Bn != B or Gn != G:
            form = f"the {G} heads', tokens (G = {G}, B = {B}, N, H)" if grouped else \
                f"a single head's, tokens (B = {B}, N, H)"
            raise RuntimeError(f"{what}: the list must be {form}, got {tuple(nbest.tokens.shape)}")
        if H > WER_MAX_LEN:
            raise ValueError(f"{what}: hypotheses of up to {H} tokens exceed the WER kernel's {WER_MAX_LEN}")
    check_on_device(None, xs[0])
    dev = xs[0].device
    table = _fusion_table(lm, dev, what)
    in_len = _dev_i32(il, dev)
    if nbest is None:
        nbest = _nbest_decode(xs, grouped, in_len, beam, n, False, (lm, lw, lb) if fusion else None, what)
    else:
        check_on_device(what, nbest.tokens, nbest.lengths, nbest.count)
    xs = [x if x.dtype == torch.float32 else x.float() for x in xs]
    loss, *rest = MWERLossOp.apply(
        in_len, _dev_i32(nbest.tokens, dev), _dev_i32(nbest.lengths, dev), _dev_i32(nbest.count, dev),
        _dev_i32(labels, dev), _dev_i32(torch.as_tensor(gloss_lengths).reshape(-1), dev), ps, reference, table, lw, lb,
        grouped, *xs)
    if not return_details:
        return loss
    details = dict(zip(("loglik", "posterior", "errors", "ref_valid", "risk"), rest))
    if not (grouped or reference):
        del details["ref_valid"]
    return loss, details


class MWER:
    """What `train_step` and `BucketedTrainStep` add to the step as `mwer=`: the MWER loss of the
    logits `head` (one of the model's five), with the list decoded per step by a beam of
    `beam_size` (1 <= beam_size <= 32) keeping `nbest` entries (default: all of the beam), the
    posterior sharpened by `posterior_scale`, and `weight` (finite, >= 0) times the loss added to
    `total_loss` for the backward.  `head` may be a tuple of distinct head names: their losses
    come from one grouped call and the step adds `weight` times their sum.  `head`, or an entry of
    the tuple (at most 8 entries), may also be an `EnsembleSpec` (distinct objects): the step
    computes that ensemble of its own logits with `differentiable=True` and takes the loss on it
    like on any head, so the gradient reaches every member; a `LearnedEnsemble` stands where an
    `EnsembleSpec` does, and its `weight_logits` takes a gradient too (the steps clear it with the
    model's).  `reference`, `lm`
    (a `BigramLM` or an `NGramLM` on the model's device, or a (C, C) table), `lm_weight`, `length_bonus` and
    `fusion` are `mwer_loss`'s: the reference as one more entry of every list, the gloss model's
    prior inside the posterior, the list from the fused search.  ValueError for anything else."""

    def __init__(self, weight, beam_size=5, nbest=None, posterior_scale=1.0, head="fuse_coord_gloss_logits", *,
                 reference=False, lm=None, lm_weight=0.0, length_bonus=0.0, fusion=False):
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
        if isinstance(head, list):
            head = tuple(head)
        names = head if isinstance(head, tuple) else (head,)
        if not 1 <= len(names) <= MAX_HEADS:
            raise ValueError(f"MWER: between 1 and {MAX_HEADS} heads, got {len(names)}")
        for name in names:
            if isinstance(name, (EnsembleSpec, LearnedEnsemble)):
                continue
            if not isinstance(name, str) or name not in _LOGITS:
                raise ValueError(f"MWER: head must be one of {_LOGITS}, an EnsembleSpec or a tuple of them, got {name!r}")
        keys = [n for n in names if isinstance(n, str)]
        specs = [id(n) for n in names if not isinstance(n, str)]
        if len(set(keys)) != len(keys) or len(set(specs)) != len(specs):
            raise ValueError(f"MWER: the heads must be distinct (keys by name, specs as objects), got {names}")
        if not isinstance(reference, bool):
            raise ValueError(f"MWER: reference must be a bool, got {reference!r}")
        self.lm, self.lm_weight, self.length_bonus = _check_prior(lm, lm_weight, length_bonus, fusion, None, "MWER")
        self.reference, self.fusion = reference, fusion
        self.beam_size, self.nbest, self.head = beam_size, beam_size if nbest is None else nbest, head
        self.heads = names  # the heads (logit keys or EnsembleSpecs) as a tuple, whatever form `head` has

    def __repr__(self):
        extra = ""  # the keyword-only arguments appear where they differ from their defaults
        for name, default in (("reference", False), ("lm", None), ("lm_weight", 0.0), ("length_bonus", 0.0),
                              ("fusion", False)):
            if getattr(self, name) is not default and getattr(self, name) != default:
                extra += f", {name}={getattr(self, name)!r}"
        return (f"MWER(weight={self.weight}, beam_size={self.beam_size}, nbest={self.nbest}, posterior_scale="
                f"{self.posterior_scale}, head={self.head!r}{extra})")


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
