"""Ensembles of the recognition heads on the HIP path (`sca_ensemble_log_probs`,
include/scatten.h): the normalised log-probabilities of the weighted mean of G heads'
posteriors, the tensor the multi-stream recognisers decode next to the single heads.

* `ensemble_log_probs(logits_list, weights=None, mode="prob", *, differentiable=False)` — one
  launch over the G logit tensors of one forward; device tensors in and out, no host read, usable
  under `torch.cuda.graph` capture.  `differentiable=True` attaches the result to the members
  (`EnsembleLogProbsOp`, `sca_ensemble_log_probs_bwd`), which makes the ensemble a tensor that
  `mwer_loss`, `MWER(head=EnsembleSpec(...))` and the CTC loss train on.  `"prob"`: the
  arithmetic mean of the posteriors; `"logprob"`: the log-linear (geometric) mean, renormalised.  Its output is a logit tensor like any other:
  `ctc_decode_device`, `ctc_decode_heads_device` and `ctc_align_heads_device` take it as it is.
* `EnsembleSpec(members, weights=None, mode="prob")` — which of the model's five logit tensors
  an ensemble averages; `check_ensembles` validates a `{output_key: EnsembleSpec}` dict against
  the decoded heads (`EvalState`, `BucketedEvalStep`, `recognize_step`), and `add_ensembles`
  computes them into a head-output dict.

* `LearnedEnsemble(members, mode="prob", init=None)` — the same with learned weights: an
  `nn.Module` whose one parameter `weight_logits` (G,) stays on the device; the weights are its
  softmax, computed inside the kernels (`sca_ensemble_log_probs_dw`, `_dw_bwd`), and
  `ensemble_log_probs(..., weight_logits=...)` is the call underneath.  Accepted wherever an
  `EnsembleSpec` is; `freeze()` gives the `EnsembleSpec` with the weights of the moment.

The reference has no ensemble; the semantics are the header's.
"""
import ctypes
import math

import torch
from torch import nn
from torch.autograd import Function

from . import _lib as L
from .decode import check_heads, check_on_device
from .model import _LOGITS
from .precision import fp32_compute

MAX_HEADS = L.EVAL_MAX_HEADS
MODES = ("prob", "logprob")


def _check_mode(mode, what):
    if mode not in MODES:
        raise ValueError(f"{what}: mode must be one of {MODES}, got {mode!r}")
    return MODES.index(mode)


def _check_weights(weights, G, what):
    """G normalised weights as Python floats (computed in double); None: equal weights."""
    if weights is None:
        return [1.0 / G] * G
    try:
        ws = [float(w) for w in weights]
    except (TypeError, ValueError):
        raise ValueError(f"{what}: weights must be None or {G} finite positive numbers, got {weights!r}") from None
    if len(ws) != G or not all(math.isfinite(w) and w > 0.0 for w in ws):
        raise ValueError(f"{what}: weights must be None or {G} finite positive numbers, got {weights!r}")
    total = math.fsum(ws)
    ws = [w / total for w in ws]
    if not all(float(ctypes.c_float(w).value) > 0.0 for w in ws):
        raise ValueError(f"{what}: weights must not vanish in fp32 once normalised, got {weights!r}")
    return ws


def _launch_forward(xs, weights, mode):
    """`sca_ensemble_log_probs` on contiguous fp32 device tensors: the new (B, T, C) output."""
    L.require_device(*xs)
    G = len(xs)
    B, T, C = xs[0].shape
    out = torch.empty_like(xs[0])
    hx, wx = L.decode_heads(xs), L.EnsembleWeights()
    for g in range(G):
        wx.w[g] = weights[g]
    L.check(L.lib().sca_ensemble_log_probs(ctypes.byref(hx), G, ctypes.byref(wx), mode, B, T, C, L.ptr(out),
                                           L.stream_handle()), "sca_ensemble_log_probs")
    return out


class EnsembleLogProbsOp(Function):
    """`sca_ensemble_log_probs` with its vector-Jacobian product (`sca_ensemble_log_probs_bwd`):
    `weights` (G normalised Python floats), `mode` (0 / 1) and the G fp32 device logits `*logits`,
    each (B, T, C).  The output is bitwise the detached call's.  The backward is one launch for
    all members; a member that needs no gradient is a null entry of the pointer table, so its
    gradient is neither computed nor written.  The weights are host constants."""

    @staticmethod
    def forward(ctx, weights, mode, *logits):
        xs = [x.contiguous() for x in logits]
        out = _launch_forward(xs, weights, mode)
        ctx.save_for_backward(out, *xs)
        ctx.weights, ctx.mode = weights, mode
        return out

    @staticmethod
    def backward(ctx, dout):
        out, *xs = ctx.saved_tensors
        G = len(xs)
        B, T, C = out.shape
        dout = dout.contiguous()
        L.require_device(dout)
        dxs = [torch.empty_like(x) if ctx.needs_input_grad[2 + g] else None for g, x in enumerate(xs)]
        hx, wx, gx = L.decode_heads(xs), L.EnsembleWeights(), L.EnsembleGrads()
        for g in range(G):
            wx.w[g] = ctx.weights[g]
            gx.dlogits[g] = None if dxs[g] is None else dxs[g].data_ptr()
        L.check(L.lib().sca_ensemble_log_probs_bwd(ctypes.byref(hx), G, ctypes.byref(wx), ctx.mode, B, T, C,
                                                   L.ptr(out), L.ptr(dout), ctypes.byref(gx), L.stream_handle()),
                "sca_ensemble_log_probs_bwd")
        return (None, None) + tuple(dxs)


def _launch_forward_dw(xs, theta, mode):
    """`sca_ensemble_log_probs_dw` on contiguous fp32 device tensors: the new (B, T, C) output."""
    L.require_device(theta, *xs)
    B, T, C = xs[0].shape
    out = torch.empty_like(xs[0])
    hx = L.decode_heads(xs)
    L.check(L.lib().sca_ensemble_log_probs_dw(ctypes.byref(hx), len(xs), L.ptr(theta), mode, B, T, C, L.ptr(out),
                                              L.stream_handle()), "sca_ensemble_log_probs_dw")
    return out


class LearnedEnsembleLogProbsOp(Function):
    """`sca_ensemble_log_probs_dw` with its vector-Jacobian product (`sca_ensemble_log_probs_dw_bwd`):
    `mode` (0 / 1), the (G,) fp32 device scores `theta` (the weights are softmax(theta), computed in
    the kernel from the tensor's current contents) and the G fp32 device logits `*logits`.  The
    output is bitwise the detached call's.  The backward gives the members' gradients as
    `EnsembleLogProbsOp` does (a member that needs none is a null entry) and, when `theta` requires
    one, d theta (G): per-row partials in a workspace, summed by a second launch in a fixed order."""

    @staticmethod
    def forward(ctx, mode, theta, *logits):
        xs = [x.contiguous() for x in logits]
        theta = theta.contiguous()
        out = _launch_forward_dw(xs, theta, mode)
        ctx.save_for_backward(out, theta, *xs)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dout):
        out, theta, *xs = ctx.saved_tensors
        G = len(xs)
        B, T, C = out.shape
        dout = dout.contiguous()
        L.require_device(dout)
        dxs = [torch.empty_like(x) if ctx.needs_input_grad[2 + g] else None for g, x in enumerate(xs)]
        dtheta = ws = None
        if ctx.needs_input_grad[1]:
            dtheta = torch.empty_like(theta)
            ws = L.workspace(L.lib().sca_ensemble_log_probs_dw_workspace_bytes(G, B, T), out.device)
        hx, gx = L.decode_heads(xs), L.EnsembleGrads()
        for g in range(G):
            gx.dlogits[g] = None if dxs[g] is None else dxs[g].data_ptr()
        L.check(L.lib().sca_ensemble_log_probs_dw_bwd(ctypes.byref(hx), G, L.ptr(theta), ctx.mode, B, T, C, L.ptr(out),
                                                      L.ptr(dout), ctypes.byref(gx), L.ptr(dtheta), L.ptr(ws),
                                                      L.stream_handle()), "sca_ensemble_log_probs_dw_bwd")
        return (None, dtheta) + tuple(dxs)


class _Ensembler(nn.Module):
    """Parameter-free module, so that fp16 / bf16 logits take the fp32 view of fp32_compute (and,
    on the differentiable path, receive their gradients in their own dtype through its casts).
    `weight_logits` (None: host `weights`) comes after the members, so the members' dtype decides
    the module's; `ensemble_log_probs` hands it over as fp32 already."""

    @fp32_compute()
    def forward(self, weights, mode, differentiable, *logits, weight_logits=None):
        if weight_logits is not None:
            if differentiable:
                return LearnedEnsembleLogProbsOp.apply(mode, weight_logits, *logits)
            return _launch_forward_dw([x.detach().contiguous() for x in logits], weight_logits.detach().contiguous(), mode)
        if differentiable:
            return EnsembleLogProbsOp.apply(weights, mode, *logits)
        return _launch_forward([x.detach().contiguous() for x in logits], weights, mode)


_ensembler = _Ensembler()


def _check_weight_logits(theta, xs, what):
    """The learned weights' scores: a floating (G,) tensor on the members' device.  ValueError
    otherwise, before any launch."""
    if not torch.is_tensor(theta):
        raise ValueError(f"{what}: weight_logits must be a ({len(xs)},) tensor, got {type(theta).__name__}")
    if theta.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"{what}: weight_logits must be fp32, fp16 or bf16, got {theta.dtype}")
    if tuple(theta.shape) != (len(xs),):
        raise ValueError(f"{what}: weight_logits must have shape ({len(xs)},), one score per member, got "
                         f"{tuple(theta.shape)}")
    if theta.device != xs[0].device:
        raise ValueError(f"{what}: weight_logits must be on the members' device {xs[0].device}, got {theta.device}")
    return theta


def ensemble_log_probs(logits_list, weights=None, mode="prob", *, weight_logits=None, differentiable=False):
    """The ensemble of G heads' posteriors as normalised log-probabilities, in one launch
    (`sca_ensemble_log_probs`).  `logits_list`: 1..8 tensors of one shape (B, T, C); `weights`:
    None (equal) or G finite positive numbers, normalised by their sum; `mode`: "prob", the
    arithmetic mean of the posteriors (log sum_g w_g softmax(x_g)), or "logprob", the log-linear
    mean renormalised (log_softmax(sum_g w_g log_softmax(x_g))).  With G = 1 both are the rows'
    log_softmax.  Returns a detached (B, T, C) device tensor; with `differentiable=True` the same
    bits attached to the members (`EnsembleLogProbsOp`: one more launch in the backward, for all
    the members that require a gradient; fp16 / bf16 members receive theirs in their own dtype).
    The host `weights` take no gradient.  No host sync; capturable, the backward too.

    `weight_logits` (instead of `weights`; giving both is a ValueError): a (G,) floating tensor of
    unconstrained scores on the members' device; the weights are softmax(weight_logits), computed
    inside the kernel from the tensor's contents at launch (`sca_ensemble_log_probs_dw`), so a
    captured graph follows every in-place change of it.  With `differentiable=True` it receives
    its gradient when it requires one (`LearnedEnsembleLogProbsOp`: the per-row partials and a
    second launch that sums them in a fixed order; an fp16 / bf16 tensor receives it in its own
    dtype)."""
    if not isinstance(differentiable, bool):
        raise ValueError(f"ensemble_log_probs: differentiable must be a bool, got {differentiable!r}")
    xs = check_heads(logits_list, "ensemble_log_probs")
    if xs[0].numel() == 0:
        raise ValueError(f"ensemble_log_probs: empty logits {tuple(xs[0].shape)}")
    if weight_logits is not None:
        if weights is not None:
            raise ValueError("ensemble_log_probs: give weights (host constants) or weight_logits (learned, on the "
                             "device), not both")
        theta = _check_weight_logits(weight_logits, xs, "ensemble_log_probs")
        m = _check_mode(mode, "ensemble_log_probs")
        check_on_device(None, xs[0])
        return _ensembler(None, m, differentiable, *xs, weight_logits=theta.float())
    ws = _check_weights(weights, len(xs), "ensemble_log_probs")
    m = _check_mode(mode, "ensemble_log_probs")
    check_on_device(None, xs[0])
    return _ensembler(ws, m, differentiable, *xs)


class EnsembleSpec:
    """One ensemble of the model's heads: `members`, 1..8 distinct keys of the five logit
    tensors (they need not be among the decoded heads), `weights` (None: equal, or one finite
    positive number per member) and `mode` ("prob" / "logprob"), as `ensemble_log_probs` takes
    them.  ValueError for anything else."""

    def __init__(self, members, weights=None, mode="prob"):
        if isinstance(members, str):
            raise ValueError(f"EnsembleSpec: members must be a sequence of logit keys, got the string {members!r}")
        members = tuple(members)
        if not 1 <= len(members) <= MAX_HEADS or len(set(members)) != len(members):
            raise ValueError(f"EnsembleSpec: members must be 1..{MAX_HEADS} distinct keys, got {members!r}")
        for k in members:
            if k not in _LOGITS:
                raise ValueError(f"EnsembleSpec: unknown member {k!r}; the logit keys are {_LOGITS}")
        _check_mode(mode, "EnsembleSpec")
        self.members, self.mode = members, mode
        self.weights = None if weights is None else tuple(_check_weights(weights, len(members), "EnsembleSpec"))

    def __repr__(self):
        return f"EnsembleSpec(members={self.members!r}, weights={self.weights!r}, mode={self.mode!r})"

    def compute(self, outputs, differentiable=False):
        return ensemble_log_probs([outputs[k] for k in self.members], self.weights, self.mode,
                                  differentiable=differentiable)


class LearnedEnsemble(nn.Module):
    """An ensemble of the model's heads whose weights are learned: one parameter `weight_logits`
    (G,) fp32, the weights being softmax(weight_logits) (`ensemble_log_probs(weight_logits=...)`).
    `members` and `mode` as `EnsembleSpec` takes and validates them; `init`: None (zeros: equal
    weights) or G finite positive numbers, the parameter starting at the log of their normalised
    values.  It stands wherever an `EnsembleSpec` does: in the `ensembles` of `EvalState`,
    `BucketedEvalStep`, `recognize_step` and `BucketedRecognizer`, and as a head of `MWER`, where
    the steps also clear its gradient.  The kernels read the parameter from device memory, so a
    captured step follows an optimizer update or `load_state_dict` without recapture.  The module
    lives outside `MSCA_Net` (whose checkpoints load unchanged); its parameter reaches the
    optimizer as `FusedAdam(list(model.parameters()) + list(ens.parameters()), ...)`, and it moves
    to the model's device like any module (`.to(device)`)."""

    def __init__(self, members, mode="prob", init=None):
        super().__init__()
        spec = EnsembleSpec(members, None, mode)
        self.members, self.mode = spec.members, spec.mode
        if init is None:
            theta = torch.zeros(len(self.members))
        else:
            ws = _check_weights(init, len(self.members), "LearnedEnsemble")
            theta = torch.tensor([math.log(w) for w in ws], dtype=torch.float32)
        self.weight_logits = nn.Parameter(theta)

    def __repr__(self):  # no host read of the parameter
        return f"LearnedEnsemble(members={self.members!r}, mode={self.mode!r})"

    def compute(self, outputs, differentiable=False):
        return ensemble_log_probs([outputs[k] for k in self.members], None, self.mode,
                                  weight_logits=self.weight_logits, differentiable=differentiable)

    def weights(self):
        """softmax(weight_logits) as a tuple of Python floats: one explicit host read."""
        theta = self.weight_logits.detach().cpu().double()
        return tuple(torch.softmax(theta, 0).tolist())

    def freeze(self):
        """The plain `EnsembleSpec` with the current weights as host constants (one host read),
        for deployment on the host-weight path."""
        return EnsembleSpec(self.members, self.weights(), self.mode)


def learned_ensembles(heads):
    """The `LearnedEnsemble`s among an `MWER`'s heads (or any sequence of keys and specs)."""
    return [h for h in heads if isinstance(h, LearnedEnsemble)]


def check_ensembles(heads, ensembles, what):
    """The `{output_key: EnsembleSpec}` dict of an evaluation or recognition step (a value may also
    be a `LearnedEnsemble`), validated on the host against the decoded `heads`: every key contains "gloss_logits" (the reference's
    evaluate_fn loop would pick it up), is none of the five logit keys, and heads plus ensembles
    are at most 8 decoded tensors.  Returns the dict (empty for None), in insertion order."""
    if ensembles is None:
        return {}
    if not isinstance(ensembles, dict):
        raise ValueError(f"{what}: ensembles must be a dict {{output_key: EnsembleSpec}}, got {type(ensembles).__name__}")
    for key, spec in ensembles.items():
        if not isinstance(key, str) or "gloss_logits" not in key:
            raise ValueError(f"{what}: an ensemble's output key must contain 'gloss_logits', got {key!r}")
        if key in _LOGITS:
            raise ValueError(f"{what}: the ensemble key {key!r} is one of the model's own logit keys {_LOGITS}")
        if not isinstance(spec, (EnsembleSpec, LearnedEnsemble)):
            raise ValueError(f"{what}: ensembles[{key!r}] must be an EnsembleSpec or a LearnedEnsemble, got "
                             f"{type(spec).__name__}")
    if len(heads) + len(ensembles) > MAX_HEADS:
        raise ValueError(f"{what}: {len(heads)} heads and {len(ensembles)} ensembles are more than the {MAX_HEADS} "
                         "tensors one grouped decode takes")
    return dict(ensembles)


def add_ensembles(outputs, ensembles):
    """Compute every ensemble of `ensembles` from the logits in `outputs` and put it there under
    its key (one launch each).  Returns the keys added, in order."""
    for key, spec in ensembles.items():
        outputs[key] = spec.compute(outputs)
    return tuple(ensembles)
