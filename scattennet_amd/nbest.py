"""The second pass over the CTC beam search, on the device: the N best labellings of the search
(`sca_ctc_beam_decode_nbest`, the interface of `tf.nn.ctc_beam_search_decoder`'s `top_paths`),
their rescoring with a bigram gloss model and a length bonus, the posterior over the list
(`sca_nbest_rescore`) and minimum-Bayes-risk selection under the project's WER alignment
(`sca_nbest_mbr`).  The semantics are the header's (include/scatten.h); the reference has none
of this.

* `ctc_decode_nbest_device` / `ctc_decode_nbest_heads_device` — an `NBest` of device tensors
  (tokens (.., N, T) int32 padded with 0, lengths (.., N), scores (.., N), count (..)), `..`
  being (B) or (G, B).  `ctc_decode_nbest` — host lists of (ids, score) with one copy.
* `ctc_decode_fused_nbest_device` / `ctc_decode_fused_nbest_heads_device` / `ctc_decode_fused_nbest` —
  the same list from the search with the bigram model inside it (shallow fusion,
  `sca_ctc_beam_decode_fused_nbest`): beams are ranked by total + lm_weight * bigram terms +
  length_bonus * len; scores stay acoustic.  `Rescoring(..., fusion=True)` selects it in the steps.
* `BigramLM` — a dense (C, C) table of log-probabilities; class 0, the blank, is the sentence
  boundary.  `BigramLM.from_sequences` estimates one with add-k smoothing on the host.
* `NGramLM` (ngram.py) — a backoff n-gram model of order 1 to 3 as a sorted trie on the device,
  taken wherever a `BigramLM` is, except by the fused search (`NGramLM.to_bigram()` gives its
  dense form).
* `rescore_nbest_device` — (total, posterior, order); `mbr_select_device` — (best, risk, loss);
  `select_device` — one entry per list as a 1-best (tokens, lengths, values) triple.
* `Rescoring` — the validated spec that `decode_and_align`, `eval_step`, `BucketedEvalStep`,
  `recognize_step`, `BucketedRecognizer` and `decode_outputs` take as `rescoring=`; `rescored_decode`
  is what they run in place of the 1-best decode.

No call reads the device or allocates outside the caching allocator: everything is usable under
`torch.cuda.graph` capture.  With `collapse_repeats` (the default, the reference's groupby) equal
entries are merged and the list re-sorted, so entry 0 may differ from `ctc_decode_device`'s result.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from .decode import MAX_BEAM, WER_MAX_LEN, _check_lengths, _check_logits, _decoder, check_heads, check_on_device
from .heads import _dev_i32
from .ngram import NGramLM

MAX_HEADS = L.EVAL_MAX_HEADS
MAX_CLASSES = 8192  # SCA_CTC_MAX_C
SELECT = ("score", "mbr")

NBest = collections.namedtuple("NBest", "tokens lengths scores count")


# ------------------------------------------------------------------------------ the decode
def _check_beam(beam_size, nbest):
    beam = int(beam_size)
    if not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"ctc_decode_nbest: beam_size must lie in [1, {MAX_BEAM}] (the greedy decoder has no "
                         f"n-best list), got {beam}")
    n = beam if nbest is None else int(nbest)
    if not 1 <= n <= beam:
        raise ValueError(f"ctc_decode_nbest: nbest must lie in [1, beam_size = {beam}], got {n}")
    return beam, n


def _nbest_decode(xs, grouped, input_lengths, beam_size, nbest, collapse_repeats, fusion=None, what=None):
    """The n-best decode behind the four wrappers below, `rescored_decode` and `mwer_loss`: `xs`
    is the validated list of logits tensors (one, with `grouped=False`, for the single-tensor
    form of the result); `fusion`: None for the plain search, or (lm, lm_weight, length_bonus)
    for the fused one, validated here under the name `what`."""
    beam, n = _check_beam(beam_size, nbest)
    B, T, C = xs[0].shape
    il = _check_lengths(input_lengths, B, T)
    lm, lw, lb = None, 0.0, 0.0
    if fusion is not None:
        lm = fusion[0]
        _dense_only(lm, what)
        lw, lb = _check_fusion(*fusion, C, what)
    check_on_device(None, xs[0])
    table = _fusion_table(lm, xs[0].device, what)
    return NBest(*_decoder("nbest" if fusion is None else "fused", _dev_i32(il, xs[0].device), beam, n,
                           bool(collapse_repeats), lw, lb, grouped, *xs, table=table))


def ctc_decode_nbest_device(gloss_logits, input_lengths, beam_size, nbest=None, collapse_repeats=True):
    """The `nbest` (default: `beam_size`) best labellings of `ctc_decode_device`'s search over
    batch-major logits (B, T, C), as an `NBest` of device tensors: tokens (B, N, T) int32 padded
    with 0, lengths (B, N), scores (B, N) (log-probabilities, descending), count (B): entries
    >= count are empty with score -inf.  With `collapse_repeats=False` entry 0 is bitwise
    `ctc_decode_device(..., collapse_repeats=False)`; with it, entries that collapse to one
    labelling are merged (logaddexp) and the list re-sorted.  No host sync; capturable."""
    _check_logits(gloss_logits)
    return _nbest_decode([gloss_logits], False, input_lengths, beam_size, nbest, collapse_repeats)


def ctc_decode_nbest_heads_device(logits_list, input_lengths, beam_size, nbest=None, collapse_repeats=True):
    """`ctc_decode_nbest_device` over the G heads of one forward in one grouped call: an `NBest`
    of tokens (G, B, N, T), lengths (G, B, N), scores (G, B, N), count (G, B); row g is bitwise
    the single-head call's for `logits_list[g]`."""
    xs = check_heads(logits_list, "ctc_decode_nbest_heads")
    return _nbest_decode(xs, True, input_lengths, beam_size, nbest, collapse_repeats)


def nbest_lists(tokens, lengths, values, count, extra=None, order=None):
    """Host arrays of one list batch (.., N, T) / (.., N) / (.., N) / (..) as nested Python lists
    of (ids, value) — (ids, value, extra) with `extra` (.., N) — over the valid entries, in
    entry order or in `order` (.., N)."""
    tokens, lengths, values, count = (np.asarray(a) for a in (tokens, lengths, values, count))
    lead = count.shape
    out = np.empty(lead, dtype=object)
    for idx in np.ndindex(*lead):
        c = int(count[idx])
        entries = [int(e) for e in (order[idx][:c] if order is not None else range(c))]
        rows = []
        for e in entries:
            ids = [int(v) for v in tokens[idx][e][:int(lengths[idx][e])]]
            rows.append((ids, float(values[idx][e])) if extra is None else
                        (ids, float(values[idx][e]), float(extra[idx][e])))
        out[idx] = rows
    return out.tolist()


def ctc_decode_nbest(gloss_logits, beam_size, input_lengths, nbest=None, collapse_repeats=True):
    """`ctc_decode` with alternatives: a list of B lists of (class ids, score), best first, with
    one device-to-host copy."""
    return _host_lists(ctc_decode_nbest_device(gloss_logits, input_lengths, beam_size, nbest, collapse_repeats))


def _host_lists(nb):
    B, N, T = nb.tokens.shape
    packed = torch.cat([nb.count.reshape(B, 1).double(), nb.lengths.double(), nb.scores.double(),
                        nb.tokens.reshape(B, N * T).double()], dim=1).cpu().numpy()  # exact for int32, fp32
    return nbest_lists(packed[:, 1 + 2 * N:].reshape(B, N, T).astype(np.int64), packed[:, 1:1 + N].astype(np.int64),
                       packed[:, 1 + N:1 + 2 * N], packed[:, 0].astype(np.int64))


# ----------------------------------------------------------------------- shallow fusion
def _dense_only(lm, what):
    """The fused search scans a dense row per beam: it takes no `NGramLM`."""
    if isinstance(lm, NGramLM):
        raise ValueError(f"{what}: the fused search takes a BigramLM (a dense table), not an NGramLM; an order-1 "
                         "or order-2 model has one: lm.to_bigram()")


def _check_fusion(lm, lm_weight, length_bonus, num_classes, what):
    """Host-side validation of a gloss model (a `BigramLM`, an `NGramLM` or None) and its weights;
    (lm_weight, length_bonus) as floats."""
    if lm is not None and not isinstance(lm, (BigramLM, NGramLM)):
        raise ValueError(f"{what}: lm must be a BigramLM, an NGramLM or None, got {type(lm).__name__}")
    lw, lb = _finite("lm_weight", lm_weight, what), _finite("length_bonus", length_bonus, what)
    if lm is not None and lm.num_classes != num_classes:
        raise ValueError(f"{what}: the gloss model has {lm.num_classes} classes, the logits {num_classes}")
    return lw, lb


def _fusion_table(lm, device, what):
    """What the ops take for a validated gloss model on the logits' device: a `BigramLM`'s table,
    an `NGramLM` itself (its struct holds the pointers), or None."""
    if lm is None:
        return None
    if lm.device != device:
        raise RuntimeError(f"{what}: the gloss model is on {lm.device}, the logits on {device}; use lm.to(device)")
    return lm if isinstance(lm, NGramLM) else lm.table


def ctc_decode_fused_nbest_device(gloss_logits, input_lengths, beam_size, lm, lm_weight=0.0, length_bonus=0.0,
                                  nbest=None, collapse_repeats=True):
    """`ctc_decode_nbest_device` with the bigram gloss model inside the search (shallow fusion,
    `sca_ctc_beam_decode_fused_nbest`): every frame keeps the `beam_size` best prefixes by
    total + lm_weight * (the prefix's bigram terms) + length_bonus * len, and the final beams are
    ordered by that key with the closing bigram added.  `lm`: a `BigramLM` on the logits' device,
    or None (the length bonus alone guides the search).  The `NBest` has the unfused call's
    format: `scores` are acoustic log-probabilities, so `rescore_nbest_device` with the same
    `lm`, `lm_weight` and `length_bonus` gives the totals the search ranked by.  With weight 0
    and bonus 0 the result is bitwise `ctc_decode_nbest_device`'s.  No host sync; capturable."""
    _check_logits(gloss_logits)
    return _nbest_decode([gloss_logits], False, input_lengths, beam_size, nbest, collapse_repeats,
                         (lm, lm_weight, length_bonus), "ctc_decode_fused_nbest")


def ctc_decode_fused_nbest_heads_device(logits_list, input_lengths, beam_size, lm, lm_weight=0.0, length_bonus=0.0,
                                        nbest=None, collapse_repeats=True):
    """`ctc_decode_fused_nbest_device` over the G heads of one forward in one grouped call, shaped
    like `ctc_decode_nbest_heads_device`'s result; row g is bitwise the single-head call's."""
    xs = check_heads(logits_list, "ctc_decode_nbest_heads")
    return _nbest_decode(xs, True, input_lengths, beam_size, nbest, collapse_repeats, (lm, lm_weight, length_bonus),
                         "ctc_decode_fused_nbest_heads")


def ctc_decode_fused_nbest(gloss_logits, beam_size, input_lengths, lm, lm_weight=0.0, length_bonus=0.0, nbest=None,
                           collapse_repeats=True):
    """`ctc_decode_nbest` over the fused search: a list of B lists of (class ids, acoustic score),
    in the list's order, with one device-to-host copy."""
    return _host_lists(ctc_decode_fused_nbest_device(gloss_logits, input_lengths, beam_size, lm, lm_weight,
                                                     length_bonus, nbest, collapse_repeats))


# ------------------------------------------------------------------------- the gloss model
class BigramLM:
    """A bigram gloss model: `table` (C, C), log-probabilities `table[prev, cur]`, kept as an fp32
    tensor (`device`: where; default the table's own, a numpy array stays on the host until
    `.to(device)`).  Class 0 is the blank and never a token, so it stands for the sentence
    boundary: `table[0, c]` opens a sentence, `table[p, 0]` closes it, and the empty hypothesis
    costs `table[0, 0]`."""

    def __init__(self, table, device=None):
        t = torch.as_tensor(table)
        if t.dim() != 2 or t.shape[0] != t.shape[1] or not 1 <= t.shape[0] <= MAX_CLASSES:
            raise ValueError(f"BigramLM: table must be (C, C) with 1 <= C <= {MAX_CLASSES}, got {tuple(t.shape)}")
        if not (t.is_floating_point() and bool(torch.isfinite(t).all())):
            raise ValueError("BigramLM: table must hold finite floating-point log-probabilities")
        self.table = t.detach().to(device=device, dtype=torch.float32).contiguous()

    @property
    def num_classes(self):
        return self.table.shape[0]

    @property
    def device(self):
        return self.table.device

    def to(self, device):
        return BigramLM(self.table, device)

    def __repr__(self):
        return f"BigramLM(C={self.num_classes}, device={self.table.device})"

    @staticmethod
    def counts(seqs, num_classes):
        """(C, C) int64 bigram counts of the sequences with a boundary (class 0) on either side;
        an empty sequence counts one (0, 0)."""
        C = int(num_classes)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"BigramLM: num_classes must lie in [1, {MAX_CLASSES}], got {num_classes}")
        n = np.zeros((C, C), np.int64)
        for seq in seqs:
            ids = [int(v) for v in seq]
            if any(not 1 <= v < C for v in ids):
                raise ValueError(f"BigramLM: tokens must lie in [1, {C}) (0 is the blank), got {ids}")
            path = [0] + ids + [0]
            for p, c in zip(path[:-1], path[1:]):
                n[p, c] += 1
        return n

    @classmethod
    def from_sequences(cls, seqs, num_classes, add_k=1.0, device=None):
        """Add-k estimate from token-id sequences (host-side numpy):
        table[p, c] = log((n[p, c] + k) / (sum_c n[p, c] + k C)); every row log-sum-exps to 0."""
        k = float(add_k)
        if not (math.isfinite(k) and k > 0.0):
            raise ValueError(f"BigramLM: add_k must be finite and positive, got {add_k!r}")
        n = cls.counts(seqs, num_classes).astype(np.float64)
        table = np.log(n + k) - np.log(n.sum(1, keepdims=True) + k * n.shape[1])
        return cls(torch.from_numpy(table), device)


# ------------------------------------------------------------------- rescore, MBR, select
def _check_nbest(nb, what):
    """(G, B, N, T) of an NBest of contiguous device tensors; a single-head list has G = 1."""
    if not (isinstance(nb, tuple) and len(nb) == 4 and all(torch.is_tensor(t) for t in nb)):
        raise RuntimeError(f"{what}: expected an NBest (tokens, lengths, scores, count) of tensors")
    tokens, lengths, scores, count = nb
    if tokens.dim() not in (3, 4) or lengths.shape != tokens.shape[:-1] or scores.shape != lengths.shape or \
            count.shape != lengths.shape[:-1]:
        raise RuntimeError(f"{what}: tokens (.., N, T), lengths and scores (.., N) and count (..) do not fit: "
                           f"{tuple(tokens.shape)}, {tuple(lengths.shape)}, {tuple(scores.shape)}, {tuple(count.shape)}")
    G = tokens.shape[0] if tokens.dim() == 4 else 1
    B, N, T = tokens.shape[-3:]
    if not (1 <= G <= MAX_HEADS and B >= 1 and 1 <= N <= MAX_BEAM and T >= 1):
        raise ValueError(f"{what}: a list batch of (G, B, N, T) = {(G, B, N, T)} is outside 1 <= G <= {MAX_HEADS}, "
                         f"B, T >= 1, 1 <= N <= {MAX_BEAM}")
    return G, B, N, T


def _i32(t):
    return t.to(torch.int32).contiguous()


def _f32(t):
    return t.detach().float().contiguous()


def _finite(name, v, what):
    v = float(v)
    if not math.isfinite(v):
        raise ValueError(f"{what}: {name} must be finite, got {v!r}")
    return v


def rescore_nbest_device(nb, lm=None, lm_weight=0.0, length_bonus=0.0, posterior_scale=1.0):
    """`sca_nbest_rescore` over an `NBest`: total = score + lm_weight * lm(h) + length_bonus *
    len(h), posterior = softmax over the valid entries of posterior_scale * total, order = the
    valid entries by total descending (ties to the lower entry), invalid entries after them.
    `lm`: a `BigramLM` or an `NGramLM` (`sca_nbest_rescore_ngram`: the backoff rule over the trie)
    on the device, or None (lm(h) = 0: the call only produces the posterior).
    Returns (total, posterior, order) shaped like `nb.scores`, fp32 / fp32 / int32."""
    what = "rescore_nbest"
    G, B, N, T = _check_nbest(nb, what)
    if lm is not None and not isinstance(lm, (BigramLM, NGramLM)):
        raise ValueError(f"{what}: lm must be a BigramLM, an NGramLM or None, got {type(lm).__name__}")
    lw, lb, ps = (_finite(n, v, what) for n, v in (("lm_weight", lm_weight), ("length_bonus", length_bonus),
                                                   ("posterior_scale", posterior_scale)))
    check_on_device(what, *nb)
    if lm is not None:
        check_on_device(what, lm.uni_lp if isinstance(lm, NGramLM) else lm.table)
    if isinstance(lm, NGramLM):
        _fusion_table(lm, nb.tokens.device, what)
    tokens, lengths, count = _i32(nb.tokens), _i32(nb.lengths), _i32(nb.count)
    scores = _f32(nb.scores)
    total, posterior = torch.empty_like(scores), torch.empty_like(scores)
    order = torch.empty_like(lengths)
    if isinstance(lm, NGramLM):
        L.check(L.lib().sca_nbest_rescore_ngram(L.ptr(tokens), L.ptr(lengths), L.ptr(scores), L.ptr(count), G, B, N, T,
                                                ctypes.byref(lm.struct), lw, lb, ps, L.ptr(total), L.ptr(posterior),
                                                L.ptr(order), L.stream_handle()), "sca_nbest_rescore_ngram")
        return total, posterior, order
    L.check(L.lib().sca_nbest_rescore(L.ptr(tokens), L.ptr(lengths), L.ptr(scores), L.ptr(count), G, B, N, T,
                                      None if lm is None else L.ptr(lm.table), 0 if lm is None else lm.num_classes,
                                      lw, lb, ps, L.ptr(total), L.ptr(posterior), L.ptr(order), L.stream_handle()),
            "sca_nbest_rescore")
    return total, posterior, order


def mbr_select_device(nb, posterior):
    """`sca_nbest_mbr`: loss (.., N, N) int32, loss[i, j] = the error count (deletions +
    insertions + substitutions of the project's WER alignment) of hypothesis i against reference
    j; risk (.., N) = sum_j posterior_j loss[i, j]; best (..) int32 = the arg-min, ties to the
    lower entry.  Returns (best, risk, loss).  T <= 128 (the WER matrix)."""
    what = "mbr_select"
    G, B, N, T = _check_nbest(nb, what)
    if T > WER_MAX_LEN:
        raise ValueError(f"{what}: hypotheses of up to {T} tokens exceed the WER kernel's {WER_MAX_LEN}")
    if not torch.is_tensor(posterior) or posterior.shape != nb.lengths.shape:
        raise RuntimeError(f"{what}: posterior must be a tensor shaped like the list's scores {tuple(nb.lengths.shape)}")
    check_on_device(what, *nb, posterior)
    tokens, lengths, count, post = _i32(nb.tokens), _i32(nb.lengths), _i32(nb.count), _f32(posterior)
    loss = torch.empty(tuple(lengths.shape) + (N,), dtype=torch.int32, device=tokens.device)
    risk = torch.empty_like(post)
    best = torch.empty_like(count)
    L.check(L.lib().sca_nbest_mbr(L.ptr(tokens), L.ptr(lengths), L.ptr(count), L.ptr(post), G, B, N, T, L.ptr(loss),
                                  L.ptr(risk), L.ptr(best), L.stream_handle()), "sca_nbest_mbr")
    return best, risk, loss


def select_device(nb, values, index):
    """`sca_nbest_gather`: one entry of every list as a 1-best triple (tokens (.., T), lengths (..),
    values (..)).  `index`: `order` (.., N) — its first column, the best total — or `best` (..)."""
    what = "select_nbest"
    G, B, N, T = _check_nbest(nb, what)
    lead = tuple(nb.count.shape)
    if tuple(index.shape) not in (lead, lead + (N,)) or values.shape != nb.lengths.shape:
        raise RuntimeError(f"{what}: index must be shaped {lead} or {lead + (N,)} and values {tuple(nb.lengths.shape)}")
    check_on_device(what, *nb, values, index)
    stride = N if index.dim() == nb.lengths.dim() else 1
    tokens, lengths, idx, val = _i32(nb.tokens), _i32(nb.lengths), _i32(index), _f32(values)
    tokens1 = torch.empty(lead + (T,), dtype=torch.int32, device=tokens.device)
    lengths1 = torch.empty(lead, dtype=torch.int32, device=tokens.device)
    values1 = torch.empty(lead, dtype=torch.float32, device=tokens.device)
    L.check(L.lib().sca_nbest_gather(L.ptr(tokens), L.ptr(lengths), L.ptr(val), L.ptr(idx), stride, G, B, N, T,
                                     L.ptr(tokens1), L.ptr(lengths1), L.ptr(values1), L.stream_handle()),
            "sca_nbest_gather")
    return tokens1, lengths1, values1


# --------------------------------------------------------------------------------- the spec
class Rescoring:
    """What the evaluation and recognition steps run in place of the 1-best decode: the `nbest`
    best labellings of the beam search (1 <= nbest <= 32, and at most the step's beam_size),
    rescored with `lm` (a `BigramLM`, an `NGramLM` or None; the spec holds it, so a captured
    graph's pointers stay alive), `lm_weight`, `length_bonus` and `posterior_scale`
    as `rescore_nbest_device` takes them, and the hypothesis picked by `select`: "score", the
    best total, or "mbr", the minimum expected error count under the posterior.  `fusion=True`:
    the list comes from the fused search (`ctc_decode_fused_nbest_heads_device` with this spec's
    `lm`, `lm_weight` and `length_bonus`), so the search keeps what the rescorer would have
    preferred; everything after the decode is unchanged.  ValueError for anything else, for
    `fusion=True` with neither a table nor a length bonus (nothing to fuse), and for `fusion=True`
    with an `NGramLM` (the fused search takes a `BigramLM`: `lm.to_bigram()`)."""

    def __init__(self, nbest, lm=None, lm_weight=0.0, length_bonus=0.0, posterior_scale=1.0, select="score",
                 fusion=False):
        if isinstance(nbest, bool) or not isinstance(nbest, int) or not 1 <= nbest <= MAX_BEAM:
            raise ValueError(f"Rescoring: nbest must be an int in [1, {MAX_BEAM}], got {nbest!r}")
        if lm is not None and not isinstance(lm, (BigramLM, NGramLM)):
            raise ValueError(f"Rescoring: lm must be a BigramLM, an NGramLM or None, got {type(lm).__name__}")
        if select not in SELECT:
            raise ValueError(f"Rescoring: select must be one of {SELECT}, got {select!r}")
        self.nbest, self.lm, self.select = nbest, lm, select
        try:
            self.lm_weight = _finite("lm_weight", lm_weight, "Rescoring")
            self.length_bonus = _finite("length_bonus", length_bonus, "Rescoring")
            self.posterior_scale = _finite("posterior_scale", posterior_scale, "Rescoring")
        except TypeError:
            raise ValueError("Rescoring: lm_weight, length_bonus and posterior_scale must be numbers") from None
        if not isinstance(fusion, bool):
            raise ValueError(f"Rescoring: fusion must be a bool, got {fusion!r}")
        if fusion:
            _dense_only(lm, "Rescoring")
        if fusion and lm is None and self.length_bonus == 0.0:
            raise ValueError("Rescoring: fusion=True needs a gloss model or a length bonus: there is nothing to fuse")
        self.fusion = fusion

    def __repr__(self):
        return (f"Rescoring(nbest={self.nbest}, lm={self.lm!r}, lm_weight={self.lm_weight}, length_bonus="
                f"{self.length_bonus}, posterior_scale={self.posterior_scale}, select={self.select!r}, "
                f"fusion={self.fusion})")

    def check(self, beam_size, num_classes, frames, what):
        """Host-side validation against a step's beam, the logits' class count and their frame
        count (None: not known yet)."""
        beam = int(beam_size)
        if not 1 <= beam <= MAX_BEAM:
            raise ValueError(f"{what}: rescoring needs a beam search, beam_size in [1, {MAX_BEAM}], got {beam}")
        if self.nbest > beam:
            raise ValueError(f"{what}: rescoring.nbest = {self.nbest} exceeds beam_size = {beam}")
        if self.lm is not None and num_classes is not None and self.lm.num_classes != num_classes:
            raise ValueError(f"{what}: the gloss model has {self.lm.num_classes} classes, the logits {num_classes}")
        if self.select == "mbr" and frames is not None and frames > WER_MAX_LEN:
            raise ValueError(f"{what}: select='mbr' over {frames} logit frames exceeds the WER kernel's "
                             f"{WER_MAX_LEN} tokens")


def check_rescoring(rescoring, beam_size, what, num_classes=None, frames=None):
    """`rescoring=` of a step, validated on the host: None, or a `Rescoring` that fits."""
    if rescoring is None:
        return None
    if not isinstance(rescoring, Rescoring):
        raise ValueError(f"{what}: rescoring must be a Rescoring or None, got {type(rescoring).__name__}")
    rescoring.check(beam_size, num_classes, frames, what)
    return rescoring


def rescored_decode(logits_list, input_lengths, beam_size, rescoring, what="rescored_decode"):
    """The grouped n-best decode of G heads (the fused search with `rescoring.fusion`), the rescore
    and (select="mbr") the MBR selection, and the selected hypothesis as a 1-best triple.  Returns a dict of device tensors: `tokens`
    (G, B, T), `lengths` (G, B), `scores` (G, B) (the selected entry's total) and the list itself:
    `nbest_tokens` (G, B, N, T), `nbest_lengths`, `nbest_totals`, `nbest_posterior`, `nbest_order`
    (G, B, N), `nbest_count` (G, B), and with "mbr" `nbest_risk` (G, B, N), `nbest_best` (G, B).
    No host read."""
    xs = check_heads(logits_list, "ctc_decode_nbest_heads")
    check_rescoring(rescoring, beam_size, what, xs[0].shape[2], xs[0].shape[1])
    fusion = (rescoring.lm, rescoring.lm_weight, rescoring.length_bonus) if rescoring.fusion else None
    nb = _nbest_decode(xs, True, input_lengths, beam_size, rescoring.nbest, True, fusion,
                       "ctc_decode_fused_nbest_heads")
    total, posterior, order = rescore_nbest_device(nb, rescoring.lm, rescoring.lm_weight, rescoring.length_bonus,
                                                   rescoring.posterior_scale)
    out = {"nbest_tokens": nb.tokens, "nbest_lengths": nb.lengths, "nbest_totals": total,
           "nbest_posterior": posterior, "nbest_order": order, "nbest_count": nb.count}
    index = order
    if rescoring.select == "mbr":
        out["nbest_best"], out["nbest_risk"], _ = mbr_select_device(nb, posterior)
        index = out["nbest_best"]
    out["tokens"], out["lengths"], out["scores"] = select_device(nb, total, index)
    return out
