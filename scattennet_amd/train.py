"""The training step of opt.py:28-38 on the device: zero_grad, forward, the non-finite test,
backward, clip_grad_norm_ and optimizer.step() with no host read in between.

`train_step(model, optimizer, src_input)` enqueues one whole step — forward with the finite
check deferred, backward of `total_loss`, `FusedAdam.step(loss=guard)` — and returns the
model's outputs.  The update is skipped on the device when any checked tensor was not finite
(`guard` is NaN then), including tensors that do not feed `total_loss`, as the reference's
`raise` would have stopped the step.  `read_report(outputs)` is the single host read:
the loss terms as Python floats plus `skipped`, raising the reference's ValueError when
flagged — by then the parameters are untouched.

Capture.  For a fixed (B, T, S) the step is capturable into one hipGraph:

1. hand `src_input` over as device tensors (their storage is what every replay reads);
2. run one eager `train_step` on a side stream (it allocates the optimizer's moments and
   tables, the library's lazy state and the dropout counter);
3. capture `train_step` with `torch.cuda.graph` and keep the returned outputs: replays refill
   the same tensors;
4. between replays, call `optimizer.sync_hyperparameters()` after a scheduler step, and
   `read_report` whenever the host wants the numbers.

Batches whose T varies: `scattennet_amd.BucketedTrainStep` (bucketed.py) follows these rules
once per length bucket and replays the bucket's graph on padded batches.
"""
import math

import torch

from . import heads, ops
from .distill import check_distill
from .ensemble import learned_ensembles
from .model import _students_of, deferred_check, first_error, flag_names, guard_of
from .model import read_report as model_read_report
from .mwer import check_mwer, mwer_guard, mwer_loss


def _add_mwer(outputs, src_input, mwer):
    """The MWER term of a step: `outputs["mwer_loss"]`, `outputs["mwer_risk"]` (B) and
    `outputs["mwer_report"]` = (mwer_loss, mean risk), the two numbers `read_report` adds to its
    one copy.  Returns the loss to back-propagate.  With a tuple of G heads, one grouped call:
    `outputs["mwer_losses"]` (G) holds each head's loss, `mwer_loss` their sum and `mwer_risk` is
    (G, B)."""
    grouped = isinstance(mwer.head, tuple)
    # an EnsembleSpec among the heads: the ensemble of this step's logits, attached to its members
    logits = [outputs[h] if isinstance(h, str) else h.compute(outputs, differentiable=True) for h in mwer.heads]
    labels = heads.labels_2d(src_input, logits[0].shape[0], "train_step")
    loss, details = mwer_loss(logits if grouped else logits[0], outputs["input_lengths"], labels,
                              src_input["gloss_lengths"], beam_size=mwer.beam_size, nbest_size=mwer.nbest,
                              posterior_scale=mwer.posterior_scale, return_details=True, reference=mwer.reference,
                              lm=mwer.lm, lm_weight=mwer.lm_weight, length_bonus=mwer.length_bonus,
                              fusion=mwer.fusion)
    if grouped:
        outputs["mwer_losses"], loss = loss, loss.sum()
    outputs["mwer_loss"], outputs["mwer_risk"] = loss, details["risk"]
    outputs["mwer_report"] = torch.stack([loss.detach(), details["risk"].mean()])
    return outputs["total_loss"] + mwer.weight * loss


def _add_distill(model, outputs, src_input, distill, loss):
    """The ensemble-distillation term of a step: `outputs["ensemble_kd_losses"]` (S), one loss per
    student of `distill` from one grouped call, `outputs["ensemble_kd_loss"]`, their sum, and
    `outputs["ensemble_kd_report"]`, the sum as a (1,) device tensor for `read_report`'s one copy.
    A batch padded to a length bucket (`valid_frames`) takes part with its valid frames only.
    Returns `loss` plus the term.  (No key ends in `_distill_loss`: the report layout of the
    model's own terms follows from that suffix.)"""
    valid = None
    if src_input.get("valid_frames") is not None:
        valid = (src_input["valid_frames"].to(outputs[distill.students[0]].device), model.n_pool())
    losses = distill.losses(outputs, valid=valid)
    total = losses.sum()
    outputs["ensemble_kd_losses"], outputs["ensemble_kd_loss"] = losses, total
    outputs["ensemble_kd_report"] = total.detach().float().reshape(1)
    return loss + total


def step_parameters(model, mwer):
    """The parameters whose gradients a step clears: the model's and, with an `MWER` that has
    `LearnedEnsemble`s among its heads, theirs (modules outside the model), so that a weight
    gradient does not accumulate across steps."""
    yield from model.parameters()
    if mwer is not None:
        for ens in learned_ensembles(mwer.heads):
            yield from ens.parameters()


def train_step(model, optimizer, src_input, mwer=None, distill=None):
    """One training step of MSCA_Net with FusedAdam, enqueued on the current stream without a
    host read.  Returns the forward's outputs (`finite_report` holds the losses and flags).
    `mwer`: None, or an `MWER`: the step decodes the chosen head's logits (or, for a tuple of heads,
    all of them in one grouped call, which also adds `mwer_losses` (G)) into an n-best list,
    adds `mwer_loss`, `mwer_risk` and `mwer_report` to the outputs (the last is the pair
    (mwer_loss, mean risk) as one device tensor, which lets `read_report` keep to a single copy) and
    back-propagates `total_loss + weight * mwer_loss`; a non-finite `mwer_loss` skips the update on the device like a flagged tensor.
    A `LearnedEnsemble` among the heads has its `weight_logits.grad` cleared with the model's and
    filled by the backward; the optimizer updates it when it was given the parameter.
    `distill`: None, or a `Distill`: its students learn from its teacher (a head, or an ensemble of
    this step's heads formed inside the kernels) in one grouped call; the step adds
    `ensemble_kd_losses` (S), `ensemble_kd_loss` (their sum) and `ensemble_kd_report`, back-propagates
    the sum with the rest, and skips the update on the device when it is not finite.  The teacher
    is detached.  It comes on top of the model's own `*_distill_loss` terms; with
    cfg["self_distillation"] = False it stands instead of them."""
    check_mwer(mwer, "train_step")
    check_distill(distill, "train_step")
    for p in step_parameters(model, mwer):
        p.grad = None
    ops.advance_dropout()
    with deferred_check(model):
        outputs = model(src_input)
    loss, guard = outputs["total_loss"], None
    if mwer is not None:
        loss = _add_mwer(outputs, src_input, mwer)
        guard = mwer_guard(guard_of(outputs), outputs["mwer_loss"])
    if distill is not None:
        loss = _add_distill(model, outputs, src_input, distill, loss)
        guard = mwer_guard(guard_of(outputs) if guard is None else guard, outputs["ensemble_kd_loss"])
    ops.fork_ledger_begin()
    try:
        loss.backward()
        # weight gradients held back for the side stream and deferred LayerNorm-affine
        # reductions are normally launched by the backward's final callback; a backward that
        # left some behind must not reach the update without them
        ops.flush_pending()
    except BaseException:
        try:
            ops.fork_ledger_end()
        except RuntimeError:
            pass  # the backward's own error is the one to report
        raise
    ops.fork_ledger_end()  # every stream forked in the step has joined the origin (capture rule)
    optimizer.step(loss=guard_of(outputs) if guard is None else guard)
    return outputs


def read_report(outputs):
    """The step's one host read: the loss terms (`total_loss`, `alignment_loss`,
    `fuse_coord_loss`, `*_distill_loss`) and `guard` as Python floats, the flag words, and
    `skipped` (the update did not happen: `guard` was not finite, the test FusedAdam makes on
    the device).  Raises the reference's ValueError (model/__init__.py:130-235) when a checked
    tensor was not finite.  After a step with `mwer=`, also `mwer_loss` and `mwer_risk` (the mean
    over the clips), from the same single copy; a non-finite `mwer_loss` counts as `skipped`.
    After a step with `distill=`, also `ensemble_kd_loss`, from that copy too and with the same rule."""
    mwer, kd = outputs.get("mwer_report"), outputs.get("ensemble_kd_report")
    if mwer is None and kd is None:
        rep = model_read_report(outputs)
        rep["skipped"] = not math.isfinite(rep["guard"])
    else:
        report = outputs["finite_report"]
        words = torch.cat([report] + [x.view(report.dtype) for x in (mwer, kd) if x is not None]).cpu()
        rep = model_read_report({**outputs, "finite_report": words[:report.numel()]})
        extra = [float(v) for v in words[report.numel():].view(torch.float32)]
        terms = []
        if mwer is not None:
            rep["mwer_loss"], rep["mwer_risk"] = extra[:2]
            terms.append(rep["mwer_loss"])
        if kd is not None:
            rep["ensemble_kd_loss"] = extra[-1]
            terms.append(extra[-1])
        rep["skipped"] = not all(math.isfinite(v) for v in [rep["guard"]] + terms)
    msg = first_error(rep["flags"], flag_names(_students_of(outputs)))
    if msg is not None:
        raise ValueError(msg)
    return rep
