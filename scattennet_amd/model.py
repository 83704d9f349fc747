"""MSCA_Net (model/__init__.py:72-290): the whole network as a drop-in module.

Same constructor, attributes, children and state_dict keys as the reference, so a reference
checkpoint loads with `strict=True`; `forward(src_input)` returns the reference's dict (the five
logit tensors, `input_lengths`, `total_loss`, `alignment_loss`, `fuse_coord_loss` and the
`*_distill_loss` terms) plus one key, `finite_report`.

Finite guard.  The reference tests the keypoints, the three stream embeddings, the fused
embedding, the five logit tensors and the loss terms with `isnan().any()` / `isinf().any()`
(model/__init__.py:130-235), each a reduction launch and a host read.  Here ONE launch
(`sca_finite_scan`) leaves a flag word per tensor, and one small launch (`sca_step_report`)
gathers the flag words and the loss terms into `finite_report`, computes `total_loss` and the
`guard` scalar (total_loss, or NaN when anything was flagged) that `FusedAdam.step(loss=...)`
tests on the device.  `model.check` selects what the host does with it:

* ``"sync"`` (default): one host read at the end of forward, then the `ValueError` the reference
  would have raised first (`first_error`).  While a stream is capturing it behaves as "defer".
* ``"defer"``: no host read; `model.raise_if_nonfinite(outputs)` reads and raises later.
* ``"off"``: no scan; the report holds zero flag words.

Length buckets.  `src_input` may carry `"valid_frames"`: an int32 device tensor of shape (1,)
holding the batch's own longest length when keypoints and mask are padded beyond it to a fixed
bucket (`pad_batch`, `BucketedTrainStep`).  The three ops through which frames behind that
length would reach the valid ones — the fusion softmax, the SeqKD terms and the BiLSTM's
reverse direction — then read it on the device, so the valid frames' outputs, the losses and
every parameter gradient are those of the unpadded batch.

Without labels.  `predict(src_input)` is `forward` up to the heads: the five logit tensors,
`input_lengths` and `finite_flags` (the flag words of the ten tensors checked before the losses,
`predict_flag_names`), no loss kernel and no label key; `recognize.py` decodes and aligns them.

The model computes in fp32 (`.half()` of the whole model is not supported; the submodules keep
their own reduced-precision paths).

Report layout (int32 words, `report_layout`): the flag words in `flag_names` order (bit 0 NaN,
bit 1 Inf), then as fp32 `alignment_loss`, `fuse_coord_loss`, the distillation terms in
`cfg["distillation_weight"]` order, `total_loss`, `guard`.
"""
import contextlib
import ctypes

import torch
from torch import nn
from torch.autograd import Function

from . import _lib as L
from . import heads, ops
from .encoder import SCAEncoder

FLAG_NAN, FLAG_INF = 1, 2
CHECK_MODES = ("sync", "defer", "off")
_LOGITS = ("alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits")


def flag_names(students=()):
    """The tensors the reference checks, in the order it checks them (model/__init__.py:130-235)."""
    return (["keypoints", "body_embed", "left_embed", "right_embed", "fuse_embed"] + list(_LOGITS) +
            ["alignment_loss", "fuse_coord_loss"] + [f"{s}_distill_loss" for s in students])


def predict_flag_names():
    """The tensors `MSCA_Net.predict` checks: those the reference tests before its losses."""
    return flag_names()[:5 + len(_LOGITS)]


def first_error(flags, names):
    """The message of the ValueError the reference raises first for these flag words (one per
    name, bit 0 NaN / bit 1 Inf), or None when every word is zero.  Pure host function."""
    for name, f in zip(names, flags):
        f = int(f)
        if not f & (FLAG_NAN | FLAG_INF):
            continue
        if name in _LOGITS:  # model/__init__.py:163-167 tests NaN first, then inf
            return f"NaN in {name}" if f & FLAG_NAN else f"inf in {name}"
        return "NaN or inf in " + ("input keypoints" if name == "keypoints" else name)
    return None


def report_layout(students=()):
    """Word offsets into `finite_report`: {"flags": (0, n), "<loss name>": offset, "guard": offset}."""
    names = flag_names(students)
    n = len(names)
    out = {"flags": (0, n), "alignment_loss": n, "fuse_coord_loss": n + 1}
    for i, s in enumerate(students):
        out[f"{s}_distill_loss"] = n + 2 + i
    out["total_loss"] = n + 2 + len(students)
    out["guard"] = n + 3 + len(students)
    out["words"] = n + 4 + len(students)
    return out


def _check_scannable(t):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError("scattennet_amd ops run only on ROCm (MI355X) fp32 tensors; got "
                           f"{getattr(t, 'device', type(t))} {getattr(t, 'dtype', '')}.  There is no CPU fallback.")
    if not t.is_contiguous():
        raise ValueError(f"finite_flags: tensors must be contiguous, got strides {t.stride()} for {tuple(t.shape)}")


def finite_flags(tensors):
    """One int32 device word per tensor: bit 0 set when it holds a NaN, bit 1 when it holds
    +-Inf (`sca_finite_scan`, one launch per 16 tensors, no host read).  Tensors must be
    contiguous fp32 device tensors."""
    tensors = list(tensors)
    for t in tensors:
        _check_scannable(t)
    if not tensors:
        raise ValueError("finite_flags: no tensors")
    flags = torch.empty(len(tensors), dtype=torch.int32, device=tensors[0].device)
    for c in range(0, len(tensors), L.GUARD_MAX_TENSORS):
        part = tensors[c:c + L.GUARD_MAX_TENSORS]
        ptrs = (ctypes.c_void_p * len(part))(*[t.data_ptr() for t in part])
        numels = (ctypes.c_long * len(part))(*[t.numel() for t in part])
        L.check(L.lib().sca_finite_scan(len(part), ptrs, numels, L.ptr(flags[c:]), L.stream_handle()),
                "sca_finite_scan")
    return flags


class StepReport(Function):
    """total_loss = fuse_coord_loss + sum of the distillation terms (model/__init__.py:207,237)
    and the report buffer, in one launch (`sca_step_report`).  Backward hands dloss to every
    term of the sum; alignment_loss is reported only (the reference leaves it out of the total)."""

    @staticmethod
    def forward(ctx, flags, nflags, alignment_loss, fuse_coord_loss, *distill):
        L.require_device(alignment_loss, fuse_coord_loss, *distill)
        total = fuse_coord_loss.new_empty(())
        report = torch.empty(nflags + 4 + len(distill), dtype=torch.int32, device=total.device)
        terms = (ctypes.c_void_p * max(len(distill), 1))(*[t.data_ptr() for t in distill])
        L.check(L.lib().sca_step_report(L.ptr(flags), nflags, L.ptr(alignment_loss), L.ptr(fuse_coord_loss),
                                        len(distill), terms, L.ptr(total), L.ptr(report), L.stream_handle()),
                "sca_step_report")
        ctx.mark_non_differentiable(report)
        ctx.n = len(distill)
        return total, report

    @staticmethod
    def backward(ctx, dloss, _dreport):
        return (None, None, None, dloss) + (dloss,) * ctx.n


class MSCA_Net(SCAEncoder):
    """model/__init__.py:72-290.  The encoder children and their lock-step forward are
    SCAEncoder's (body_encoder, left_encoder, right_encoder, coordinates_fusion)."""

    def __init__(self, cfg, gloss_tokenizer, device="cpu"):
        super().__init__(cfg)
        self.device = device
        self.cfg["fuse_idx"] = cfg["left_idx"] + cfg["right_idx"] + cfg["body_idx"]
        self.left_idx = cfg["left_idx"]
        self.gloss_tokenizer = gloss_tokenizer
        self.self_distillation = cfg["self_distillation"]
        self.gradient_clip_val = cfg.get("gradient_clip_val", 1.0)
        self.recognition_head = heads.RecognitionHead(cfg, gloss_tokenizer)
        self.loss_fn = nn.CTCLoss(reduction="none", zero_infinity=True, blank=0)  # kept for its attribute;
        self.distillation_loss = heads.SeqKD()                                      # the losses run in HIP
        self.check = "sync"
        self._init_weights()

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)

    def _students(self):
        return list(self.cfg["distillation_weight"]) if self.self_distillation else []

    def flag_names(self):
        return flag_names(self._students())

    def report_layout(self):
        return report_layout(self._students())

    def compute_loss(self, labels, tgt_lengths, logits, input_lengths):
        return heads.compute_loss(labels, tgt_lengths, logits, input_lengths)

    def _ctc_targets(self, host, src, B, T, C, device):
        """Labels and lengths as int32 device tensors, shared by both CTC losses.  They are
        validated once, on the host, when the caller handed them over as host tensors; device
        tensors are trusted (the kernels' clamps keep a bad call in bounds) — no host read."""
        labels = torch.as_tensor(host["gloss_labels"])
        tgt, inl = host["gloss_lengths"], host["valid_len_in"]
        on_host = all(torch.as_tensor(t).device.type == "cpu" for t in (labels, tgt, inl))
        if labels.dim() == 1:
            labels = heads._pad_concatenated(labels, tgt, B)
        elif not on_host:
            labels = src["gloss_labels"]
        if on_host:
            heads._validate_ctc(labels, tgt, inl, B, T, C)
        else:
            tgt, inl = src["gloss_lengths"], src["valid_len_in"]
        return heads._dev_i32(labels, device), heads._dev_i32(inl, device), heads._dev_i32(tgt, device)

    def forward(self, src_input, **kwargs):
        if self.check not in CHECK_MODES:
            raise ValueError(f"MSCA_Net.check must be one of {CHECK_MODES}, got {self.check!r}")
        host = src_input
        if torch.cuda.is_available() and self.device == "cuda":
            src_input = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in src_input.items()}
        keypoints = src_input["keypoints"]
        mask = src_input["mask"]
        valid = None
        if src_input.get("valid_frames") is not None:
            if torch.compiler.is_compiling():
                raise NotImplementedError("MSCA_Net: valid_frames (length-bucketed batches) is not supported while "
                                          "torch.compile traces; run the bucketed step eagerly or captured")
            valid = ops.check_valid((src_input["valid_frames"], self.n_pool()))

        fuse_embed, left_embed, right_embed, body_embed = self.encode(keypoints, mask, valid=valid)
        head_outputs = self.recognition_head(left_embed, right_embed, fuse_embed, body_embed, valid=valid)
        outputs = {k: head_outputs[k] for k in _LOGITS if k in head_outputs}
        outputs["input_lengths"] = src_input["valid_len_in"]

        fuse_logits = outputs["fuse_coord_gloss_logits"]
        B, T, C = fuse_logits.shape
        labels, in_len, tgt_len = self._ctc_targets(host, src_input, B, T, C, fuse_logits.device)
        outputs["alignment_loss"] = heads.CTCLossOp.apply(outputs["alignment_gloss_logits"], labels, in_len,
                                                          tgt_len)[0]
        outputs["fuse_coord_loss"] = heads.CTCLossOp.apply(fuse_logits, labels, in_len, tgt_len)[0]
        students = self._students()
        for student in students:
            outputs[f"{student}_distill_loss"] = heads.distillation_loss(
                outputs[student], fuse_logits, self.cfg["distillation_weight"][student], valid=valid)

        names = self.flag_names()
        flags = None
        if self.check != "off":
            scanned = {"keypoints": keypoints, "body_embed": body_embed, "left_embed": left_embed,
                       "right_embed": right_embed, "fuse_embed": fuse_embed}
            flags = finite_flags([(scanned[n] if n in scanned else outputs[n]).detach().contiguous() for n in names])
        total, report = StepReport.apply(flags, len(names), outputs["alignment_loss"].detach(),
                                         outputs["fuse_coord_loss"], *[outputs[f"{s}_distill_loss"] for s in students])
        outputs["total_loss"] = total
        outputs["finite_report"] = report
        if self.check == "sync" and not torch.cuda.is_current_stream_capturing():
            self.raise_if_nonfinite(outputs)
        return outputs

    def predict_flag_names(self):
        return predict_flag_names()

    def predict(self, src_input):
        """The label-free forward: `forward`'s `encode` and `recognition_head` calls and nothing
        after them.  `src_input` needs `keypoints`, `mask`, `valid_len_in` and, for a batch padded
        to a bucket, `valid_frames`; no label key is read and no loss kernel is launched.  Returns
        the five logit tensors, `input_lengths` and `finite_flags`: the int32 device words of
        `finite_flags()` over the ten tensors the reference checks before its losses
        (`predict_flag_names()`), all zero with `check == "off"`.  `check == "sync"` reads them once
        and raises the reference's ValueError (`first_error`); "defer" and a capturing stream make
        no host read (`raise_if_flagged(outputs["finite_flags"])` later)."""
        if self.check not in CHECK_MODES:
            raise ValueError(f"MSCA_Net.check must be one of {CHECK_MODES}, got {self.check!r}")
        if torch.cuda.is_available() and self.device == "cuda":
            src_input = {k: v.cuda() if isinstance(v, torch.Tensor) else v for k, v in src_input.items()}
        keypoints = src_input["keypoints"]
        mask = src_input["mask"]
        valid = None
        if src_input.get("valid_frames") is not None:
            if torch.compiler.is_compiling():
                raise NotImplementedError("MSCA_Net: valid_frames (length-bucketed batches) is not supported while "
                                          "torch.compile traces; run the bucketed step eagerly or captured")
            valid = ops.check_valid((src_input["valid_frames"], self.n_pool()))

        fuse_embed, left_embed, right_embed, body_embed = self.encode(keypoints, mask, valid=valid)
        head_outputs = self.recognition_head(left_embed, right_embed, fuse_embed, body_embed, valid=valid)
        outputs = {k: head_outputs[k] for k in _LOGITS if k in head_outputs}
        outputs["input_lengths"] = src_input["valid_len_in"]

        names = predict_flag_names()
        if self.check == "off":
            outputs["finite_flags"] = torch.zeros(len(names), dtype=torch.int32, device=keypoints.device)
            return outputs
        scanned = {"keypoints": keypoints, "body_embed": body_embed, "left_embed": left_embed,
                   "right_embed": right_embed, "fuse_embed": fuse_embed}
        outputs["finite_flags"] = finite_flags([(scanned[n] if n in scanned else outputs[n]).detach().contiguous()
                                                for n in names])
        if self.check == "sync" and not torch.cuda.is_current_stream_capturing():
            raise_if_flagged(outputs["finite_flags"])
        return outputs

    def read_report(self, outputs):
        return read_report(outputs)

    def guard(self, outputs):
        return guard_of(outputs)

    def raise_if_nonfinite(self, outputs):
        """Read the report (one host read) and raise the reference's ValueError when flagged."""
        return raise_if_nonfinite(outputs)


@contextlib.contextmanager
def deferred_check(model):
    """For the body, `model.check` is "defer" (an "off" stays "off"): what a step that must not
    read the host runs its forward under.  The earlier value is back afterwards, also when the
    body raises."""
    check, model.check = model.check, ("off" if model.check == "off" else "defer")
    try:
        yield
    finally:
        model.check = check


def _students_of(outputs):
    return [k[:-len("_distill_loss")] for k in outputs if k.endswith("_distill_loss")]


def read_report(outputs):
    """The single host read of a forward's `finite_report`: {"flags": [...], "<loss name>":
    float, ..., "guard": float}.  The layout follows from the outputs' own keys."""
    lay = report_layout(_students_of(outputs))
    words = outputs["finite_report"].cpu()
    vals = words.view(torch.float32)
    out = {"flags": words[:lay["flags"][1]].tolist()}
    for k, o in lay.items():
        if k not in ("flags", "words"):
            out[k] = float(vals[o])
    return out


def guard_of(outputs):
    """0-d fp32 device view of the report's guard scalar, for FusedAdam.step(loss=...)."""
    return outputs["finite_report"].view(torch.float32)[report_layout(_students_of(outputs))["guard"]]


def raise_if_flagged(flags):
    """One host read of `predict`'s `finite_flags`; the reference's ValueError when flagged."""
    msg = first_error(flags.cpu().tolist(), predict_flag_names())
    if msg is not None:
        raise ValueError(msg)


def raise_if_nonfinite(outputs):
    rep = read_report(outputs)
    msg = first_error(rep["flags"], flag_names(_students_of(outputs)))
    if msg is not None:
        raise ValueError(msg)
    return rep
