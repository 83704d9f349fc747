"""Evaluation on the HIP path: CTC decoding of the recognition-head logits and WER counts.

The reference's `evaluate_fn` (opt.py:50-128) copies every `*gloss_logits` tensor to the host,
runs `tf.nn.ctc_beam_search_decoder` there (utils.py:164-189) and scores the strings with
`metrics.wer_list` (metrics.py:2754-2907).  Here the logits stay where `RecognitionHead`
left them:

* `ctc_decode_device` / `ctc_greedy_decode_device` — `sca_ctc_beam_decode` /
  `sca_ctc_greedy_decode`: (tokens, lengths, scores) as device tensors, no host sync, usable
  under `torch.cuda.graph` capture (the workspace comes from the caching allocator).
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
import torch
from torch import nn

from . import _lib as L
from .heads import _dev_i32
from .precision import fp32_compute

MAX_BEAM = 32
WER_MAX_LEN = 128


def _check_logits(gloss_logits):
    if not torch.is_tensor(gloss_logits) or gloss_logits.dim() != 3:
        raise RuntimeError("ctc_decode: gloss_logits must be a (B, T, C) tensor, batch-major")


def _check_device(gloss_logits):
    if not gloss_logits.is_cuda:
        raise RuntimeError("scattennet_amd ops run only on ROCm (MI355X) tensors; got "
                           f"{gloss_logits.device} {gloss_logits.dtype}.  There is no CPU fallback.")


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


class _Decoder(nn.Module):
    """Parameter-free module, so that fp16 / bf16 logits take the fp32 view of fp32_compute."""

    @fp32_compute()
    def forward(self, logits, in_len, beam, collapse):
        x = logits.detach().contiguous()
        L.require_device(x)
        B, T, C = x.shape
        lib = L.lib()
        nbytes = lib.sca_ctc_decode_workspace_bytes(B, T, C, max(beam, 1))
        tokens = torch.empty(B, T, dtype=torch.int32, device=x.device)
        lengths = torch.empty(B, dtype=torch.int32, device=x.device)
        scores = x.new_empty(B)
        ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=x.device)
        if beam == 0:
            L.check(lib.sca_ctc_greedy_decode(L.ptr(x), L.ptr(in_len), B, T, C, L.ptr(tokens), L.ptr(lengths),
                                              L.ptr(scores), L.ptr(ws), L.stream_handle()), "sca_ctc_greedy_decode")
        else:
            L.check(lib.sca_ctc_beam_decode(L.ptr(x), L.ptr(in_len), B, T, C, beam, int(collapse), L.ptr(tokens),
                                            L.ptr(lengths), L.ptr(scores), L.ptr(ws), L.stream_handle()),
                    "sca_ctc_beam_decode")
        return tokens, lengths, scores


_decoder = _Decoder()


def _decode(gloss_logits, input_lengths, beam, collapse):
    _check_logits(gloss_logits)
    B, T, C = gloss_logits.shape
    if beam and not 1 <= beam <= MAX_BEAM:
        raise ValueError(f"ctc_decode: beam_size must lie in [1, {MAX_BEAM}], got {beam}")
    il = _check_lengths(input_lengths, B, T)
    _check_device(gloss_logits)
    return _decoder(gloss_logits, _dev_i32(il, gloss_logits.device), beam, collapse)


def ctc_decode_device(gloss_logits, input_lengths, beam_size=1, collapse_repeats=True):
    """CTC prefix beam search (include/scatten.h, sca_ctc_beam_decode) over batch-major logits
    (B, T, C).  Returns (tokens (B, T) int32 padded with 0, lengths (B,) int32, scores (B,):
    the log-probability of the returned labelling) on the device.  collapse_repeats merges
    adjacent equal labels of the result, as the reference's groupby does (utils.py:185-188)."""
    return _decode(gloss_logits, input_lengths, int(beam_size), bool(collapse_repeats))


def ctc_greedy_decode_device(gloss_logits, input_lengths):
    """Best-path decoding: per-frame arg-max (ties to the lowest class), repeats collapsed,
    blanks dropped; scores are the best path's log-probabilities."""
    return _decode(gloss_logits, input_lengths, 0, True)


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
        dec = {}
        for k, v in outputs.items():
            if "gloss_logits" in k:
                res = rescored_decode([v], il, beam_size, rescoring, "decode_outputs")
                dec[k.replace("gloss_logits", "")] = (res["tokens"][0], res["lengths"][0], res["scores"][0])
        return {k: _to_lists(t, n) for k, (t, n, _) in dec.items()}
    dec = {k.replace("gloss_logits", ""): ctc_decode_device(v, il, beam_size)
           for k, v in outputs.items() if "gloss_logits" in k}
    return {k: _to_lists(t, n) for k, (t, n, _) in dec.items()}


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
