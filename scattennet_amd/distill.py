"""Ensemble distillation on the HIP path (`sca_distill_heads_fwd/bwd`, include/scatten.h): the
SeqKD loss of several students against the ensemble of G heads, in one grouped call.

* `ensemble_distillation_loss(students, members, student_weights, ...)` — the S losses
  `distillation_loss(students[s], ensemble_log_probs(members, ...), student_weights[s])`, with the
  teacher formed inside the kernels and never stored: two launches in the forward and one in the
  backward whatever G and S are.  With one member it is bitwise `distillation_loss` per student,
  the reference's own distillation (model/__init__.py:203-214) for all students at once.  The
  teacher is detached, as the reference's is: only the students take a gradient.
* `Distill(teacher, students, T=1.0)` — what `train_step` and `BucketedTrainStep` add to the step
  as `distill=`: `teacher` is one of the model's logit keys, an `EnsembleSpec` or a
  `LearnedEnsemble`; `students` maps logit keys to their weights.

The reference distils from the single `fuse_coord_gloss_logits` head only; the ensemble teacher
is the on-the-fly ensemble distillation recipe on top of it, and the semantics are the header's.
"""
import ctypes
import math

import torch
from torch import nn
from torch.autograd import Function

from . import _lib as L
from . import ops
from .decode import check_heads, check_on_device
from .ensemble import EnsembleSpec, LearnedEnsemble, _check_mode, _check_weight_logits, _check_weights
from .model import _LOGITS
from .precision import fp32_compute

MAX_STUDENTS = L.DISTILL_MAX_STUDENTS


class EnsembleDistillOp(Function):
    """`sca_distill_heads_fwd` with its backward (`sca_distill_heads_bwd`).  `cfg` = (S, G, mode,
    weights, student_weights, start, temp, lo, hi, valid): `weights` the G normalised host weights
    or None, with which `theta`, the (G,) fp32 device scores, is read by the kernels; `valid` None
    or (valid_frames, shift).  `*tensors`: the S students, then the G members, fp32 (B, T, C) on
    the device.  Returns the (S,) losses.  Only the students take a gradient; one that needs none
    is a null entry of the pointer table, so nothing of it is computed or written."""

    @staticmethod
    def forward(ctx, cfg, theta, *tensors):
        S, G, mode, weights, student_weights, start, temp, lo, hi, valid = cfg
        xs = [x.contiguous() for x in tensors]
        theta = None if theta is None else theta.contiguous()
        L.require_device(theta, *xs)
        B, T, C = xs[0].shape
        lib = L.lib()
        losses = xs[0].new_empty(S)
        ws = xs[0].new_empty(max(lib.sca_distill_heads_workspace_floats(S, G, B, T), 1))
        ctx.tables = _tables(xs[:S], xs[S:], weights, student_weights)
        hx, wx, sx = ctx.tables
        vf, shift = (None, 0) if valid is None else valid
        L.check(lib.sca_distill_heads_fwd(ctypes.byref(hx), G, None if wx is None else ctypes.byref(wx), L.ptr(theta),
                                          mode, ctypes.byref(sx), S, B, T, C, start, temp, lo, hi, L.ptr(vf), shift,
                                          L.ptr(losses), L.ptr(ws), L.stream_handle()), "sca_distill_heads_fwd")
        ctx.save_for_backward(ws, *xs, *(() if theta is None else (theta,)))
        ctx.cfg = cfg  # valid_frames is not a saved tensor: an input the host rewrites between replays
        return losses

    @staticmethod
    def backward(ctx, dlosses):
        S, G, mode, weights, _, start, temp, _lo, _hi, valid = ctx.cfg
        ws, *xs = ctx.saved_tensors
        theta = None if weights is not None else xs.pop()
        B, T, C = xs[0].shape
        dlosses = dlosses.contiguous()
        L.require_device(dlosses)
        dxs = [torch.empty_like(xs[s]) if ctx.needs_input_grad[2 + s] else None for s in range(S)]
        hx, wx, sx = ctx.tables
        gx = L.DistillGrads()
        for s in range(S):
            gx.dlogits[s] = None if dxs[s] is None else dxs[s].data_ptr()
        vf, shift = (None, 0) if valid is None else valid
        L.check(L.lib().sca_distill_heads_bwd(ctypes.byref(hx), G, None if wx is None else ctypes.byref(wx),
                                              L.ptr(theta), mode, ctypes.byref(sx), S, B, T, C, start, temp,
                                              L.ptr(vf), shift, L.ptr(dlosses), L.ptr(ws), ctypes.byref(gx),
                                              L.stream_handle()), "sca_distill_heads_bwd")
        return (None, None) + tuple(dxs) + (None,) * G


def _tables(students, members, weights, student_weights):
    """The by-value tables of one call: members, host weights (None with device scores), students."""
    hx, sx, wx = L.decode_heads(members), L.DistillStudents(), None
    if weights is not None:
        wx = L.EnsembleWeights()
        for g, w in enumerate(weights):
            wx.w[g] = w
    for s, x in enumerate(students):
        sx.logits[s] = x.data_ptr()
        sx.weight[s] = student_weights[s]
    return hx, wx, sx


class _Distiller(nn.Module):
    """Parameter-free module, so that fp16 / bf16 logits take the fp32 view of fp32_compute and the
    students receive their gradients in their own dtype through its casts (as `_Ensembler`)."""

    @fp32_compute()
    def forward(self, cfg, *tensors, weight_logits=None):
        S = cfg[0]
        tensors = tensors[:S] + tuple(x.detach() for x in tensors[S:])  # the teacher is detached
        return EnsembleDistillOp.apply(cfg, None if weight_logits is None else weight_logits.detach(), *tensors)


_distiller = _Distiller()


def _check_student_weights(weights, S, what):
    try:
        ws = [float(w) for w in weights]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: student_weights must be {S} finite numbers >= 0, got {weights!r}") from None
    if len(ws) != S or not all(math.isfinite(w) and w >= 0.0 for w in ws):
        raise ValueError(f"{what}: student_weights must be {S} finite numbers >= 0, got {weights!r}")
    return ws


def _check_temperature(T, what):
    if isinstance(T, bool) or not isinstance(T, (int, float)) or not math.isfinite(T) or not T > 0:
        raise ValueError(f"{what}: the temperature T must be a finite number > 0, got {T!r}")
    return float(T)


def ensemble_distillation_loss(students, members, student_weights, *, weights=None, weight_logits=None, mode="prob",
                               T=1.0, use_blank=False, clamp=(-100.0, 100.0), valid=None):
    """The (S,) losses clamp(student_weights[s] * SeqKD(T)(students[s], e.detach(), use_blank), *clamp)
    with e = `ensemble_log_probs(members, weights, mode, weight_logits=...)`, in one grouped call
    (`sca_distill_heads_fwd`; the backward is one launch for all students that require a gradient).
    `students`: 1..8 tensors (B, T, C), `members`: 1..8 tensors of the same shape, dtype and
    device; a student may be one of the members.  `weights` / `weight_logits`, `mode`: as
    `ensemble_log_probs` takes them (neither: equal weights).  `valid=(valid_frames, shift)`: as
    `distillation_loss` takes it.  The teacher is detached: neither the members nor
    `weight_logits` take a gradient from this term.  With one member the result is bitwise
    `distillation_loss(students[s], members[0], ...)` per student.  No host sync; capturable."""
    what = "ensemble_distillation_loss"
    ss = list(students)
    if not 1 <= len(ss) <= MAX_STUDENTS:
        raise ValueError(f"{what}: between 1 and {MAX_STUDENTS} students, got {len(ss)}")
    xs = check_heads(members, what)
    ss = check_heads(ss, what)
    check_heads([ss[0], xs[0]], what)  # the students have the members' shape, dtype and device
    if xs[0].numel() == 0:
        raise ValueError(f"{what}: empty logits {tuple(xs[0].shape)}")
    sw = _check_student_weights(student_weights, len(ss), what)
    temp = _check_temperature(T, what)
    if not isinstance(use_blank, bool):
        raise ValueError(f"{what}: use_blank must be a bool, got {use_blank!r}")
    start = 0 if use_blank else 1
    if start >= xs[0].shape[-1]:
        raise ValueError(f"{what}: use_blank=False needs more than one class, got C = {xs[0].shape[-1]}")
    try:
        lo, hi = (float(v) for v in clamp)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: clamp must be a pair (lo, hi) of numbers, got {clamp!r}") from None
    if not lo <= hi:
        raise ValueError(f"{what}: clamp must be a pair lo <= hi, got {clamp!r}")
    m = _check_mode(mode, what)
    theta = ws = None
    if weight_logits is not None:
        if weights is not None:
            raise ValueError(f"{what}: give weights (host constants) or weight_logits (learned, on the device), "
                             "not both")
        theta = _check_weight_logits(weight_logits, xs, what).float()
    else:
        ws = tuple(_check_weights(weights, len(xs), what))
    check_on_device(None, xs[0])
    if valid is not None:
        valid = ops.check_valid(valid)
    cfg = (len(ss), len(xs), m, ws, tuple(sw), start, temp, lo, hi, valid)
    return _distiller(cfg, *ss, *xs, weight_logits=theta)


class Distill:
    """What `train_step` and `BucketedTrainStep` add to the step as `distill=`: the students
    `students`, a dict {logit key: weight} of 1..8 of the model's five logit tensors with finite
    weights >= 0, learn from `teacher` at temperature `T` (> 0): one of the logit keys (the
    reference's own distillation, whatever the head), an `EnsembleSpec` or a `LearnedEnsemble` of
    this step's logits.  The teacher is detached; a `LearnedEnsemble`'s `weight_logits` is read on
    the device, so a captured step follows its updates (MWER on the ensemble trains it).
    ValueError for anything else."""

    def __init__(self, teacher, students, T=1.0):
        if not (isinstance(teacher, (EnsembleSpec, LearnedEnsemble)) or (isinstance(teacher, str) and teacher in _LOGITS)):
            raise ValueError(f"Distill: teacher must be one of {_LOGITS}, an EnsembleSpec or a LearnedEnsemble, got "
                             f"{teacher!r}")
        if not isinstance(students, (dict, list, tuple)):
            raise ValueError(f"Distill: students must be a dict {{logit key: weight}}, got {type(students).__name__}")
        pairs = list(students.items()) if isinstance(students, dict) else [tuple(p) for p in students]
        if not 1 <= len(pairs) <= MAX_STUDENTS:
            raise ValueError(f"Distill: between 1 and {MAX_STUDENTS} students, got {len(pairs)}")
        keys = [p[0] for p in pairs]
        for k in keys:
            if not isinstance(k, str) or k not in _LOGITS:
                raise ValueError(f"Distill: unknown student {k!r}; the logit keys are {_LOGITS}")
        if len(set(keys)) != len(keys):
            raise ValueError(f"Distill: the students must be distinct, got {keys!r}")
        for p in pairs:
            if len(p) != 2 or isinstance(p[1], bool) or not isinstance(p[1], (int, float)):
                raise ValueError(f"Distill: a student's weight must be a number, got {p!r}")
        self.weights = tuple(_check_student_weights([p[1] for p in pairs], len(pairs), "Distill"))
        self.T = _check_temperature(T, "Distill")
        self.teacher, self.students = teacher, tuple(keys)

    def __repr__(self):
        return f"Distill(teacher={self.teacher!r}, students={dict(zip(self.students, self.weights))!r}, T={self.T})"

    def losses(self, outputs, valid=None):
        """The (S,) losses on a step's head outputs, one grouped call."""
        t = self.teacher
        if isinstance(t, str):
            members, kw = [outputs[t]], {}
        elif isinstance(t, LearnedEnsemble):
            members, kw = [outputs[k] for k in t.members], {"weight_logits": t.weight_logits, "mode": t.mode}
        else:
            members, kw = [outputs[k] for k in t.members], {"weights": t.weights, "mode": t.mode}
        return ensemble_distillation_loss([outputs[k] for k in self.students], members, self.weights, T=self.T,
                                          valid=valid, **kw)


def check_distill(distill, what):
    """`distill=` of a step, validated on the host: None or a `Distill`."""
    if distill is not None and not isinstance(distill, Distill):
        raise ValueError(f"{what}: distill must be a Distill or None, got {type(distill).__name__}")
    return distill
