"""CTC forced alignment on the HIP path: when each gloss of a label sequence was signed and how
sure the head was (`sca_ctc_align_heads`, include/scatten.h).

The recognition heads' batch-major logits (B, T, C) stay on the device; for a label sequence per
clip (the references, or a decoder's own hypotheses) the Viterbi path through the extended CTC
states gives, per label, its frame span [start, end) and the mean posterior over that span.

* `ctc_align_heads_device` — the G heads of one forward in one grouped call, against labels
  shared by the heads (B, S) or one set per head (G, B, S).  Device tensors in and out, no host
  read, usable under `torch.cuda.graph` capture (the workspace comes from the caching allocator).
* `ctc_align_device` — the G = 1 form.
* `ctc_align` — the same with one device-to-host copy: per clip a list of
  (class id, start, end, confidence); `align_outputs` — that over every `*gloss_logits` key of a
  head-output dict, as `decode_outputs` decodes them.
* `alignment_lists` — the pure host conversion.

Blank is class 0.  Lengths and labels given as CPU tensors are validated on the host, device
tensors are trusted (the kernel clamps lengths and label values to stay in bounds), as in
decode.py.  The reference has no forced alignment; the semantics are the header's.
"""
import collections
import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib as L
from .decode import _check_lengths, _check_logits, check_heads, check_on_device
from .heads import _dev_i32
from .precision import fp32_compute

MAX_HEADS = L.EVAL_MAX_HEADS
MAX_LABELS = 1023  # SCA_CTC_MAX_S
MAX_CLASSES = 8192  # SCA_CTC_MAX_C

Alignment = collections.namedtuple("Alignment", ["frame_label", "spans", "conf", "scores"])


class _HeadsAligner(nn.Module):
    """Parameter-free module, so that fp16 / bf16 logits take the fp32 view of fp32_compute."""

    @fp32_compute()
    def forward(self, in_len, labels, lab_len, per_head, *logits):
        xs = [x.detach().contiguous() for x in logits]
        L.require_device(*xs)
        G = len(xs)
        B, T, C = xs[0].shape
        S = labels.shape[-1]
        lib = L.lib()
        nbytes = lib.sca_ctc_align_workspace_bytes(G, B, T, S)
        dev = xs[0].device
        frame_label = torch.empty(G, B, T, dtype=torch.int32, device=dev)
        spans = torch.empty(G, B, S, 2, dtype=torch.int32, device=dev)
        conf = xs[0].new_empty(G, B, S)
        scores = xs[0].new_empty(G, B)
        ws, hx = L.workspace(nbytes, dev), L.decode_heads(xs)
        L.check(lib.sca_ctc_align_heads(ctypes.byref(hx), G, L.ptr(in_len), L.ptr(labels), L.ptr(lab_len),
                                        int(per_head), B, T, C, S, L.ptr(frame_label), L.ptr(spans), L.ptr(conf),
                                        L.ptr(scores), L.ptr(ws), L.stream_handle()), "sca_ctc_align_heads")
        return frame_label, spans, conf, scores


_heads_aligner = _HeadsAligner()


def _check_labels(labels, label_lengths, G, B, C):
    """(labels, label_lengths, per_head) validated: CPU tensors against S and [1, C), device
    tensors by shape only."""
    lab = torch.as_tensor(labels)
    if lab.dim() == 2:
        per_head, lead = False, (B,)
    elif lab.dim() == 3:
        per_head, lead = True, (G, B)
    else:
        raise RuntimeError("ctc_align: labels must be (B, S), shared by the heads, or (G, B, S), one set per head")
    if tuple(lab.shape[:-1]) != lead:
        raise RuntimeError(f"ctc_align: labels must be {lead + ('S',)} for these logits, got {tuple(lab.shape)}")
    S = lab.shape[-1]
    if S > MAX_LABELS:
        raise ValueError(f"ctc_align: label rows of {S} entries exceed the kernel's {MAX_LABELS}")
    if C > MAX_CLASSES:
        raise ValueError(f"ctc_align: {C} classes exceed the kernel's {MAX_CLASSES}")
    n = torch.as_tensor(label_lengths)
    want = G * B if per_head else B
    if n.numel() != want:
        raise RuntimeError(f"Expected label_lengths to have {want} entries (one per label row), got {n.numel()}")
    n = n.reshape(lead)
    if n.device.type == "cpu" and want:
        if int(n.max()) > S:
            raise RuntimeError(f"Expected label_lengths to have value at most {S}, but got value {int(n.max())}")
        if int(n.min()) < 0:
            raise RuntimeError(f"Expected label_lengths to be non-negative, but got value {int(n.min())}")
        if lab.device.type == "cpu" and S:
            inside = torch.arange(S).expand(lab.shape) < n.unsqueeze(-1)
            bad = inside & ((lab < 1) | (lab >= C))
            if bool(bad.any()):
                raise ValueError(f"ctc_align: labels must lie in [1, {C}) (0 is the blank), got value "
                                 f"{int(lab[bad][0])}")
    return lab, n, per_head


def ctc_align_heads_device(logits_list, input_lengths, labels, label_lengths):
    """Forced alignment of the G heads of one forward in one grouped call (`sca_ctc_align_heads`).
    `logits_list`: 1..8 tensors of one shape (B, T, C), aligned with `input_lengths` (B) against
    `labels` (B, S) / `label_lengths` (B), shared by all heads, or (G, B, S) / (G, B), one set per
    head.  Returns the named tuple (frame_label (G, B, T) int32: the label index emitted at each
    frame, -1 at blanks and beyond the clip; spans (G, B, S, 2) int32: [start, end) per label;
    conf (G, B, S): the mean posterior of the label over its span; scores (G, B): the path's
    log-probability, -inf for a clip that cannot emit its labels) on the device: row g is bitwise
    what the single-head call returns.  No host sync; capturable."""
    xs = check_heads(logits_list, "ctc_align_heads")
    B, T, C = xs[0].shape
    il = _check_lengths(input_lengths, B, T)
    lab, n, per_head = _check_labels(labels, label_lengths, len(xs), B, C)
    check_on_device(None, xs[0])
    dev = xs[0].device
    return Alignment(*_heads_aligner(_dev_i32(il, dev), _dev_i32(lab, dev), _dev_i32(n, dev), per_head, *xs))


def ctc_align_device(gloss_logits, input_lengths, labels, label_lengths):
    """`ctc_align_heads_device` for one head: labels (B, S), label_lengths (B); the results
    without the leading head dimension."""
    _check_logits(gloss_logits)
    if torch.as_tensor(labels).dim() != 2:
        raise RuntimeError("ctc_align: labels must be (B, S) for one head")
    return Alignment(*(t[0] for t in ctc_align_heads_device([gloss_logits], input_lengths, labels, label_lengths)))


def alignment_lists(labels, label_lengths, spans, conf, scores, frame_scale=1):
    """Pure host function on arrays of one head: labels (B, S), label_lengths (B), spans
    (B, S, 2), conf (B, S), scores (B).  Per clip a list of (class id, start * frame_scale,
    end * frame_scale, confidence), one entry per label (an empty list for no labels), or None
    for an infeasible clip (score -inf).  `frame_scale`: input frames per logit frame (the
    encoder's temporal pooling), to report spans in input frames."""
    labels, n = np.asarray(labels), np.asarray(label_lengths).reshape(-1)
    spans, conf, scores = np.asarray(spans), np.asarray(conf, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    out = []
    for b in range(len(n)):
        if np.isneginf(scores[b]):
            out.append(None)
            continue
        out.append([(int(labels[b, j]), int(spans[b, j, 0]) * frame_scale, int(spans[b, j, 1]) * frame_scale,
                     float(conf[b, j])) for j in range(int(n[b]))])
    return out


def _host(*tensors):
    """One device-to-host copy of several (rows, ...) tensors: packed as float64 columns (exact
    for int32 and fp32), split again on the host."""
    rows = tensors[0].shape[0]
    flat = [t.reshape(rows, -1).to(torch.float64) for t in tensors]
    packed = torch.cat(flat, dim=1).cpu().numpy()
    out, at = [], 0
    for t, f in zip(tensors, flat):
        out.append(packed[:, at:at + f.shape[1]].reshape(tuple(t.shape)))
        at += f.shape[1]
    return out


def ctc_align(gloss_logits, input_lengths, labels, label_lengths, frame_scale=1):
    """Forced alignment of one head with one device-to-host copy: per clip a list of
    (class id, start, end, confidence), None for an infeasible clip (`alignment_lists`)."""
    res = ctc_align_device(gloss_logits, input_lengths, labels, label_lengths)
    dev = res.spans.device
    lab = _dev_i32(torch.as_tensor(labels), dev)
    n = _dev_i32(torch.as_tensor(label_lengths).reshape(-1), dev)
    lab_h, n_h, spans, conf, scores = _host(lab, n, res.spans, res.conf, res.scores)
    return alignment_lists(lab_h.astype(np.int64), n_h.astype(np.int64), spans.astype(np.int64), conf, scores,
                           frame_scale)


def align_outputs(outputs, labels, label_lengths, frame_scale=1):
    """The loop of `decode_outputs` for alignment: every key of `outputs` that contains
    "gloss_logits" is aligned with outputs["input_lengths"] against the shared `labels` (B, S) /
    `label_lengths` (B) in one grouped call; {logits_name: lists as `ctc_align` returns them}."""
    keys = [k for k in outputs if "gloss_logits" in k]
    res = ctc_align_heads_device([outputs[k] for k in keys], outputs["input_lengths"], labels, label_lengths)
    dev = res.spans.device
    G = len(keys)
    lab = _dev_i32(torch.as_tensor(labels), dev)
    n = _dev_i32(torch.as_tensor(label_lengths).reshape(-1), dev)
    B = lab.shape[0]
    lab_h, n_h, spans, conf, scores = _host(lab, n, res.spans.transpose(0, 1).reshape(B, -1),
                                            res.conf.transpose(0, 1).reshape(B, -1), res.scores.t())
    S = lab.shape[1]
    spans, conf = spans.reshape(B, G, S, 2).astype(np.int64), conf.reshape(B, G, S)
    return {k.replace("gloss_logits", ""): alignment_lists(lab_h.astype(np.int64), n_h.astype(np.int64), spans[:, g],
                                                           conf[:, g], scores[:, g], frame_scale)
            for g, k in enumerate(keys)}
