"""Evaluation on the HIP path: CTC decoding of the recognition-head logits and WER counts.

The reference's `evaluate_fn` (opt.py:50-128) copies every `*gloss_logits` tensor to the host,
runs `tf.nn.ctc_beam_search_decoder` there (utils.py:164-189) and scores the strings with
`metrics.wer_list` (metrics.py:2754-2907).  Here the logits stay where `RecognitionHead`
left them:

* `ctc_decode_device` / `ctc_greedy_decode_device` — `sca_ctc_beam_decode` /
  `sca_ctc_greedy_decode`: (tokens, lengths, scores) as device tensors, no host sync, usable
  under `torch.cuda.graph` capture (the workspace comes from the caching allocator).
* `ctc_decode_heads_device` — `sca_ctc_beam_decode_heads` / `sca_ctc_greedy_decode_heads`: the
  G logit tensors of one forward decoded together, bitwise what `ctc_decode_device` gives per
  head.  One module (`_Decoder`) makes these calls and the n-best and fused ones of nbest.py.
* `ctc_decode` — the reference's `utils.ctc_decode` signature and return type (a list of B
  lists of Python ints) with one device-to-host copy; `decode_outputs` — the loop of
  opt.py:76-89 over a head-output dict.
* `wer_counts` — `sca_wer_counts`: (N, 4) int32 (num_del, num_ins, num_sub, num_ref) per
  pair on the device; `wer_from_counts` — the rates of `metrics.wer_list`.

Blank is class 0: the reference rotates the blank column to the end for TensorFlow and adds 1
to TensorFlow's ids, which cancel, so the ids are the model's own class indices.  Lengths given
as CPU tensors are validated on the host (one per clip, none above T), device tensors are
trusted (the kernels clamp them to [0, T]), as in heads.py.
"""
import ctypes

import torch
from torch import nn

from . import _lib as L
from .heads import _dev_i32
from .precision import fp32_compute

MAX_BEAM = 32
MAX_HEADS = L.EVAL_MAX_HEADS
WER_MAX_LEN = 128


def _check_logits(gloss_logits):
    if not torch.is_tensor(gloss_logits) or gloss_logits.dim() != 3:
        raise RuntimeError("ctc_decode: gloss_logits must be a (B, T, C) tensor, batch-major")


def check_heads(logits_list, what):
    """The 1..8 logit tensors of one grouped call (`what`: the caller's name in the messages) as
    a list: all (B, T, C), of one shape, dtype and device."""
    xs = list(logits_list)
    if not 1 <= len(xs) <= MAX_HEADS:
        raise ValueError(f"{what}: between 1 and {MAX_HEADS} logit tensors, got {len(xs)}")
    for x in xs:
        _check_logits(x)
    first = xs[0]
    for x in xs[1:]:
        if x.shape != first.shape or x.dtype != first.dtype or x.device != first.device:
            raise ValueError(f"{what}: every head must have the same shape, dtype and device; got "
                             f"{tuple(first.shape)} {first.dtype} {first.device} and {tuple(x.shape)} {x.dtype} "
                             f"{x.device}")
    return xs


def check_on_device(what, *tensors):
    """RuntimeError for a tensor that is not on a ROCm device; `what` (or None) fronts the message."""
    front = "" if what is None else f"{what}: "
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(f"{front}scattennet_amd ops run only on ROCm (MI355X) tensors; got {t.device} "
                               f"{t.dtype}.  There is no CPU fallback.")


def _check_lengths(input_lengths, B, T):
    t = torch.as_tensor(input_lengths)
    if t.numel() != B:
        raise RuntimeError(f"Expected input_lengths to have {B} entries (one per clip), got {t.numel()}")
    if t.device.type == "cpu" and B:
        if int(t.max()) > T:
            raise RuntimeError(f"Expected input_lengths to have value at most {T}, but got value {int(t.max())}")
        if int(t.min()) < 0:
            raise RuntimeError(f"Expected input_lengths to be non-negative, but got value {int(t.min())}")
    return t.reshape(-1)


def _check_beam_size(beam):
    if beam and not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"ctc_decode: beam_size must lie in [1, {MAX_BEAM}], got {beam}")


# (mode, grouped) -> the C entry point: a single-head Python call takes the single-head symbol
_ENTRY = {("greedy", False): "sca_ctc_greedy_decode", ("greedy", True): "sca_ctc_greedy_decode_heads",
          ("beam", False): "sca_ctc_beam_decode", ("beam", True): "sca_ctc_beam_decode_heads",
          ("nbest", False): "sca_ctc_beam_decode_nbest", ("nbest", True): "sca_ctc_beam_decode_heads_nbest",
          ("fused", False): "sca_ctc_beam_decode_fused_nbest",
          ("fused", True): "sca_ctc_beam_decode_heads_fused_nbest"}


class _Decoder(nn.Module):
    """Every CTC decoder call.  Parameter-free module, so that fp16 / bf16 logits take the fp32 view
    of fp32_compute; `table` is a keyword so that the logits decide the module's dtype.

    `mode`: "greedy", "beam", "nbest" or "fused"; `nbest`, `lm_weight`, `length_bonus` and `table`
    where the mode takes them.  `grouped`: the G `logits` in one call, outputs led by (G, B);
    otherwise the single-head entry point on `logits[0]`, outputs led by (B,).  Returns (tokens,
    lengths, scores), and count for the two list modes."""

    @fp32_compute()
    def forward(self, mode, in_len, beam, nbest, collapse, lm_weight, length_bonus, grouped, *logits, table=None):
        xs = [x.detach().contiguous() for x in logits]
        L.require_device(*xs)
        G = len(xs)
        B, T, C = xs[0].shape
        lib, dev = L.lib(), xs[0].device
        lead = (G, B) if grouped else (B,)
        entry = lead + (nbest,) if mode in ("nbest", "fused") else lead  # one hypothesis, or a list of them
        out = (torch.empty(entry + (T,), dtype=torch.int32, device=dev),
               torch.empty(entry, dtype=torch.int32, device=dev), xs[0].new_empty(entry))
        if entry != lead:
            out += (torch.empty(lead, dtype=torch.int32, device=dev),)
        ws = L.workspace(lib.sca_ctc_decode_heads_workspace_bytes(G, B, T, C, max(beam, 1)), dev)
        hx = L.decode_heads(xs)
        head = (ctypes.byref(hx), G) if grouped else (L.ptr(xs[0]),)
        search = {"greedy": (), "beam": (beam, int(collapse)), "nbest": (beam, nbest, int(collapse)),
                  "fused": (beam, nbest, int(collapse), L.ptr(table), lm_weight, length_bonus)}[mode]
        name = _ENTRY[mode, grouped]
        L.check(getattr(lib, name)(*head, L.ptr(in_len), B, T, C, *search, *map(L.ptr, out), L.ptr(ws),
                                   L.stream_handle()), name)
        return out


_decoder = _Decoder()


def _decode(logits, input_lengths, beam, collapse, grouped):
    _check_beam_size(beam)
    B, T, _ = logits[0].shape
    il = _check_lengths(input_lengths, B, T)
    check_on_device(None, logits[0])
    return _decoder("beam" if beam else "greedy", _dev_i32(il, logits[0].device), beam, 0, collapse, 0.0, 0.0,
                    grouped, *logits)


def ctc_decode_device(gloss_logits, input_lengths, beam_size=1, collapse_repeats=True):
    """CTC prefix beam search (include/scatten.h, sca_ctc_beam_decode) over batch-major logits
    (B, T, C).  Returns (tokens (B, T) int32 padded with 0, lengths (B,) int32, scores (B,):
    the log-probability of the returned labelling) on the device.  collapse_repeats merges
    adjacent equal labels of the result, as the reference's groupby does (utils.py:185-188)."""
    _check_logits(gloss_logits)
    return _decode([gloss_logits], input_lengths, int(beam_size), bool(collapse_repeats), False)


def ctc_greedy_decode_device(gloss_logits, input_lengths):
    """Best-path decoding: per-frame arg-max (ties to the lowest class), repeats collapsed,
    blanks dropped; scores are the best path's log-probabilities."""
    _check_logits(gloss_logits)
    return _decode([gloss_logits], input_lengths, 0, True, False)


def ctc_decode_heads_device(logits_list, input_lengths, beam_size=1, collapse_repeats=True):
    """`ctc_decode_device` over the G heads of one forward in one grouped call
    (`sca_ctc_beam_decode_heads`; `beam_size=0`: `sca_ctc_greedy_decode_heads`).  `logits_list`:
    1..8 tensors of one shape (B, T, C), all decoded with `input_lengths` (B).  Returns (tokens
    (G, B, T) int32 padded with 0, lengths (G, B) int32, scores (G, B)) on the device: row g is
    bitwise what the single-head call returns for `logits_list[g]`.  No host sync; capturable."""
    return _decode(check_heads(logits_list, "ctc_decode_heads"), input_lengths, int(beam_size),
                   bool(collapse_repeats), True)


def _to_lists(tokens, lengths):
    packed = torch.cat([lengths.reshape(-1, 1), tokens], dim=1).cpu()  # the one device-to-host copy
    return [row[1:1 + int(row[0])].tolist() for row in packed]


def ctc_decode(gloss_logits, beam_size, input_lengths):
    """utils.ctc_decode (utils.py:164-189): a list of B lists of class ids."""
    tokens, lengths, _ = ctc_decode_device(gloss_logits, input_lengths, beam_size)
    return _to_lists(tokens, lengths)


def decode_outputs(outputs, beam_size=1, ensembles=None, rescoring=None):
    """The decoding loop of evaluate_fn (opt.py:76-89): every key of `outputs` that contains
    "gloss_logits" is decoded with outputs["input_lengths"]; the result is keyed by the
    reference's logits_name (the key without "gloss_logits").  `ensembles`
    ({output_key: EnsembleSpec}, ensemble.py) are computed from the logits in `outputs` first and
    decoded with the rest; `outputs` itself is not modified.  `rescoring` (a `Rescoring`,
    nbest.py): every tensor's hypothesis is the one selected from its rescored n-best list."""
    if ensembles is not None:
        from .ensemble import add_ensembles, check_ensembles
        outputs = dict(outputs)
        add_ensembles(outputs, check_ensembles((), ensembles, "decode_outputs"))
    il = outputs["input_lengths"]
    if rescoring is not None:
        from .nbest import rescored_decode
    dec = {}  # every decode is enqueued before the first host copy
    for k, v in outputs.items():
        if "gloss_logits" in k:
            if rescoring is not None:
                res = rescored_decode([v], il, beam_size, rescoring, "decode_outputs")
                dec[k.replace("gloss_logits", "")] = res["tokens"][0], res["lengths"][0]
            else:
                dec[k.replace("gloss_logits", "")] = ctc_decode_device(v, il, beam_size)[:2]
    return {k: _to_lists(t, n) for k, (t, n) in dec.items()}


def wer_counts(ref, ref_len, hyp, hyp_len):
    """(N, 4) int32 device counts (num_del, num_ins, num_sub, num_ref) of metrics.wer_single for
    the padded token rows ref (N, Rmax) / hyp (N, Hmax) with lengths (N,); Rmax, Hmax <= 128
    (wider rows raise ValueError: slice the padding off).  Takes the decoders' (tokens, lengths) as they are — no host read in between."""
    if not (torch.is_tensor(ref) and torch.is_tensor(hyp) and ref.dim() == 2 and hyp.dim() == 2):
        raise RuntimeError("wer_counts: ref and hyp must be (N, L) padded token tensors")
    if not (ref.is_cuda and hyp.is_cuda):
        raise RuntimeError(f"scattennet_amd ops run only on ROCm (MI355X) tensors; got {ref.device}, "
                           f"{hyp.device}.  There is no CPU fallback.")
    N = ref.shape[0]
    if hyp.shape[0] != N:
        raise RuntimeError(f"wer_counts: {N} references, {hyp.shape[0]} hypotheses")
    lens = []
    for name, t, width in (("ref_len", ref_len, ref.shape[1]), ("hyp_len", hyp_len, hyp.shape[1])):
        t = torch.as_tensor(t)
        if t.numel() != N:
            raise RuntimeError(f"Expected {name} to have {N} entries (one per pair), got {t.numel()}")
        if t.device.type == "cpu" and N and (int(t.max()) > width or int(t.min()) < 0):
            raise RuntimeError(f"Expected {name} to lie in [0, {width}]")
        lens.append(_dev_i32(t.reshape(-1), ref.device))

    r, h = ref.to(torch.int32).contiguous(), hyp.to(torch.int32).contiguous()
    counts = torch.empty(N, 4, dtype=torch.int32, device=ref.device)
    if N:
        L.check(L.lib().sca_wer_counts(L.ptr(r), L.ptr(lens[0]), L.ptr(h), L.ptr(lens[1]), N, r.shape[1], h.shape[1],
                                       L.ptr(counts), L.stream_handle()), "sca_wer_counts")
    return counts


def wer_from_counts(counts):
    """metrics.wer_list (metrics.py:2754-2790) from (N, 4) counts: totals over the pairs, each
    zero total replaced by 1, rates in percent of the reference length."""
    c = torch.as_tensor(counts).reshape(-1, 4).to(torch.int64).sum(0).tolist()
    n_del, n_ins, n_sub, n_ref = c
    n_err = n_del + n_ins + n_sub
    n_ref, n_err, n_del, n_ins, n_sub = [v if v != 0 else 1 for v in (n_ref, n_err, n_del, n_ins, n_sub)]
    return {"wer": (n_err / n_ref) * 100, "del_rate": (n_del / n_ref) * 100, "ins_rate": (n_ins / n_ref) * 100,
            "sub_rate": (n_sub / n_ref) * 100}
