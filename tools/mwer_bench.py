"""Time the MWER loss (scattennet_amd/mwer.py) on one MI355X at the evaluation shape of the 2014T
yaml (B = 8, T/4 = 64, C = 1124), beam 5 and N = 5, with the lists the decoder gives, beside what
the CTC loss of the same build costs on the same logits:

* `mwer`            MWERLossOp forward + backward over the decoder's N-best list (one tensor,
                    everything off: `sca_mwer_heads_fwd` / `_bwd` at G = 1 without the prior)
* `ctc_1target`     CTCLossOp forward + backward, one target per clip (entry 0 of the list)
* `ctc_replicated`  CTCLossOp forward + backward on logits.repeat_interleave(N, 0) with the N
                    hypotheses as labels: what the existing kernels charge for the N likelihoods
                    (the replication included); it does not deliver the MWER gradient
* `wer_pairs`       wer_counts on the B N (reference, entry) pairs: the alignment alone, which the
                    MWER forward contains and neither CTC route does
* `decode_nbest`    the uncollapsed n-best decode that a training step adds in front

Every op is a captured graph replayed in windows that take turns (tools/decode_bench.alternated):
us per call, median, min and max of --repeats windows of --steps replays, each window ending in a
device synchronise.  Synthetic logits N(0, 4^2), full-length clips, references = entry 1 of each
clip's list (so the error counts differ).  Also the statistics of the loss on these inputs: the mean
risk, the share of clips with non-constant error counts and the share of non-zero gradient rows.
Needs a GPU.

--reference, --lm, --heads G time the extended loss (the reference as a list entry, the bigram table
inside the posterior, G tensors in one grouped call) beside its yardsticks instead: see `extended`.
--ngram ORDER (with --lm implied) adds `mwer_ngram`, the loss with an `NGramLM` of that order
(`sca_mwer_heads_fwd_ngram`; tools/nbest_bench.ngram_model on the same lists) beside `mwer_lm`, and
the forwards alone (`*_fwd`, under no_grad), which is where the prior runs.
--ensemble G times the loss on the differentiable ensemble of G member tensors beside the loss on the
torch composition of the same members (autograd through log_softmax / stack / logsumexp): see `on_ensemble`.
--dump PATH saves the plain loss's outputs and gradient, for a bit-for-bit comparison of two builds
(SCA_LIB_PATH selects the library).

Usage: python tools/mwer_bench.py [--B 8] [--T 64] [--C 1124] [--beam 5] [--nbest 5] [--steps 200]
                                  [--reference] [--lm] [--ngram ORDER] [--heads G] [--ensemble G] [--dump PATH]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.decode_bench import alternated, graphed  # noqa: E402


def statistics_of(S, z, il, ref, ref_len, nb):
    """The loss on the benchmark's inputs: host numbers only (the autograd graph dies with the call)."""
    N = nb.tokens.shape[1]
    loss, det = S.mwer_loss(z, il, ref, ref_len, nbest=nb, return_details=True)
    loss.backward()
    err = det["errors"].float()
    live = torch.arange(N, device=z.device)[None, :] < nb.count[:, None]
    hi = torch.where(live, err, err.new_full((), -1e9)).max(1).values
    lo = torch.where(live, err, err.new_full((), 1e9)).min(1).values
    return {"loss": round(float(loss.detach()), 6), "risk_mean": round(float(det["risk"].mean()), 4),
            "count_mean": round(float(nb.count.float().mean()), 2),
            "clips_with_non_constant_errors": round(float((hi != lo).float().mean()), 4),
            "gradient_rows_non_zero": round(float((z.grad.abs().amax(-1) > 0).float().mean()), 4)}


def extended(a, S, dev):
    """--reference / --lm / --heads: the extended loss beside its yardsticks, forward + backward,
    captured graphs in alternated windows.  Lists: the decoder's own; references: entry 1 of each
    list with its middle token replaced by a class the list's clip does not use there (a
    reference that is NOT in the list, so the slot is valid everywhere).
    * `mwer`             the plain loss at N entries (one tensor, everything off)
    * `mwer_reference`   reference=True at N entries              (--reference)
    * `mwer_n_plus_1`    the plain loss over a list of N + 1 entries: the slot's yardstick
    * `mwer_lm`          the table on, everything else as the widest variant above   (--lm)
    * `mwer_ngram`       the same with the backoff n-gram model in place of the table  (--ngram ORDER)
    * `mwer_fwd`, `mwer_lm_fwd`, `mwer_ngram_fwd`  the forwards alone, under no_grad     (--ngram ORDER)
    * `mwer_heads`       one grouped call over G tensors                             (--heads G)
    * `mwer_calls`       G single calls on the same tensors"""
    g = torch.Generator().manual_seed(0)
    G, N = max(a.heads, 1), a.nbest
    xs = [(torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev) for _ in range(G)]
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    nbs = [S.ctc_decode_nbest_device(x, il, a.beam, N, collapse_repeats=False) for x in xs]
    nb6 = S.ctc_decode_nbest_device(xs[0], il, max(a.beam, N + 1), N + 1, collapse_repeats=False)
    pick = min(1, N - 1)
    ref_len = nbs[0].lengths[:, pick].contiguous()
    R = max(int(ref_len.max()), 1)
    ref = nbs[0].tokens[:, pick, :R].clone()
    mid = (ref_len // 2).clamp(max=R - 1).long()[:, None]
    ref.scatter_(1, mid, (ref.gather(1, mid) % (a.C - 1)) + 1)  # another class in [1, C)
    lm = None
    if a.lm:
        lm = S.BigramLM(torch.log_softmax(torch.randn(a.C, a.C, generator=g) * 2, -1), dev)
    kw = dict(reference=a.reference, lm=lm, lm_weight=0.7 if a.lm else 0.0, length_bonus=0.3 if a.lm else 0.0)
    heads_nb = S.NBest(*(torch.stack(t) for t in zip(*nbs)))

    def leaves():
        return [x.detach().clone().requires_grad_(True) for x in xs]

    def single(nb, zs=None, **kw):
        zs = zs or leaves()[:1]

        def fn():
            zs[0].grad = None
            S.mwer_loss(zs[0], il, ref, ref_len, nbest=nb, **kw).backward()
        return fn

    fns = {"mwer": single(nbs[0])}
    if a.reference:
        fns["mwer_reference"] = single(nbs[0], reference=True)
        fns["mwer_n_plus_1"] = single(nb6)
    if a.lm:
        fns["mwer_lm"] = single(nbs[0], **kw)
    sizes = None
    if a.ngram:
        from tools.nbest_bench import ngram_model, ngram_outcomes
        ng, sizes = ngram_model(S, a.ngram, a.C, nbs[0], dev)
        sizes["outcomes"] = ngram_outcomes(ng, nbs[0])
        fns["mwer_ngram"] = single(nbs[0], **dict(kw, lm=ng))

        def forward(**kw):
            def fn():
                with torch.no_grad():
                    S.mwer_loss(xs[0], il, ref, ref_len, nbest=nbs[0], **kw)
            return fn

        fns["mwer_fwd"], fns["mwer_lm_fwd"] = forward(reference=a.reference), forward(**kw)
        fns["mwer_ngram_fwd"] = forward(**dict(kw, lm=ng))
    if G > 1:
        zg, zc = leaves(), leaves()

        def mwer_heads():
            for z in zg:
                z.grad = None
            S.mwer_loss(zg, il, ref, ref_len, nbest=heads_nb, **kw).sum().backward()

        def mwer_calls():
            for z, nb in zip(zc, nbs):
                z.grad = None
                S.mwer_loss(z, il, ref, ref_len, nbest=nb, **kw).backward()

        fns["mwer_heads"], fns["mwer_calls"] = mwer_heads, mwer_calls
    replays = {}
    for name, fn in fns.items():
        replays[name] = graphed(fn)
        for _ in range(a.warmup):
            replays[name]()
    timed = alternated(replays, a.steps, a.repeats)
    z = leaves()[0]
    loss, det = S.mwer_loss(z, il, ref, ref_len, nbest=nbs[0], return_details=True, **kw)
    loss.backward()
    stats = {"loss": round(float(loss.detach()), 6), "risk_mean": round(float(det["risk"].mean()), 4),
             "gradient_rows_non_zero": round(float((z.grad.abs().amax(-1) > 0).float().mean()), 4)}
    if a.reference:
        stats["ref_valid_share"] = round(float(det["ref_valid"].float().mean()), 4)
    res = {"workload": "extended MWER loss forward + backward beside its yardsticks, graph replays", "B": a.B, "T": a.T,
           "C": a.C, "beam": a.beam, "nbest": N, "heads": G, "reference": a.reference, "lm": a.lm, "R": R,
           "steps": a.steps, "repeats": a.repeats, "unit": "us per call", "statistics": stats, "graph": timed}
    if sizes:
        res["ngram"] = sizes
        res["ngram_fwd_minus_lm_fwd"] = round(timed["mwer_ngram_fwd"]["median"] - timed["mwer_lm_fwd"]["median"], 2)
    if G > 1:
        res["heads_over_calls"] = round(timed["mwer_heads"]["median"] / timed["mwer_calls"]["median"], 3)
    print(json.dumps(res))


def on_ensemble(a, S, dev):
    """--ensemble G: MWER forward + backward on the ensemble of G members, in both modes, one list per
    mode (the decoder's, on the detached ensemble) and the references of `extended`; captured graphs in
    alternated windows, every variant on leaves of its own.
    * `op_<mode>`      ensemble_log_probs(members, differentiable=True) -> mwer_loss -> backward: the
                       ensemble's forward and its one backward launch around the loss
    * `torch_<mode>`   the torch composition of the same members -> mwer_loss -> backward
    * `loss_<mode>`    mwer_loss -> backward on the ensemble as a leaf: the loss alone"""
    from tools.ensemble_bench import torch_composition
    g = torch.Generator().manual_seed(0)
    G, N = a.ensemble, a.nbest
    xs = [(torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev) for _ in range(G)]
    weights = [1.0 / G] * G
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    kw = dict(reference=a.reference)
    fns, diff, stats = {}, {}, {}

    def leaves():
        return [x.detach().clone().requires_grad_(True) for x in xs]

    for mode in ("prob", "logprob"):
        ens = S.ensemble_log_probs(xs, None, mode)
        nb = S.ctc_decode_nbest_device(ens, il, a.beam, N, collapse_repeats=False)
        pick = min(1, N - 1)
        ref_len = nb.lengths[:, pick].contiguous()
        R = max(int(ref_len.max()), 1)
        ref = nb.tokens[:, pick, :R].clone()
        mid = (ref_len // 2).clamp(max=R - 1).long()[:, None]
        ref.scatter_(1, mid, (ref.gather(1, mid) % (a.C - 1)) + 1)  # another class in [1, C)

        def chain(form, zs, mode=mode, nb=nb, ref=ref, ref_len=ref_len):
            def fn():
                for z in zs:
                    z.grad = None
                y = zs[0] if form == "loss" else S.ensemble_log_probs(zs, None, mode, differentiable=True) \
                    if form == "op" else torch_composition(zs, weights, mode)
                loss = S.mwer_loss(y, il, ref, ref_len, nbest=nb, **kw)
                loss.backward()
                return loss.detach(), [z.grad for z in zs]
            return fn

        side = torch.cuda.Stream()  # the comparison and the statistics, off the default stream
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            (lo, go), (lt, gt) = chain("op", leaves())(), chain("torch", leaves())()
            diff[mode] = {"loss": float((lo - lt).abs()), "gradients": max(float((p - q).abs().max()) for p, q in zip(go, gt))}
            stats[mode] = {"loss": round(float(lo), 6),
                           "gradient_rows_non_zero": round(float((go[0].abs().amax(-1) > 0).float().mean()), 4)}
        torch.cuda.current_stream().wait_stream(side)
        fns[f"op_{mode}"] = chain("op", leaves())
        fns[f"torch_{mode}"] = chain("torch", leaves())
        fns[f"loss_{mode}"] = chain("loss", [ens.clone().requires_grad_(True)])
    replays = {}
    for name, fn in fns.items():
        replays[name] = graphed(fn)
        for _ in range(a.warmup):
            replays[name]()
    timed = alternated(replays, a.steps, a.repeats)
    res = {"workload": "MWER loss forward + backward on the differentiable ensemble beside the torch composition "
                       "of the same members, graph replays", "B": a.B, "T": a.T, "C": a.C, "beam": a.beam, "nbest": N,
           "members": G, "reference": a.reference, "steps": a.steps, "repeats": a.repeats, "unit": "us per call",
           "statistics": stats, "max_abs_diff_op_vs_torch": diff, "graph": timed}
    for mode in ("prob", "logprob"):
        res[f"torch_over_op_{mode}"] = round(timed[f"torch_{mode}"]["median"] / timed[f"op_{mode}"]["median"], 3)
        res[f"op_minus_loss_{mode}"] = round(timed[f"op_{mode}"]["median"] - timed[f"loss_{mode}"]["median"], 2)
        res[f"torch_minus_loss_{mode}"] = round(timed[f"torch_{mode}"]["median"] - timed[f"loss_{mode}"]["median"], 2)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ensemble", type=int, default=0, help="time the loss on the differentiable ensemble of G "
                    "members beside the loss on their torch composition (with --reference: the slot on)")
    ap.add_argument("--reference", action="store_true", help="time reference=True beside N and N + 1 entries")
    ap.add_argument("--lm", action="store_true", help="time the bigram table inside the posterior")
    ap.add_argument("--ngram", type=int, default=0, help="time an NGramLM of this order inside the posterior beside "
                    "the bigram table (implies --lm)")
    ap.add_argument("--heads", type=int, default=1, help="time one grouped call over G tensors beside G calls")
    ap.add_argument("--dump", default=None, help="save the plain loss's outputs and dlogits here (torch.save), to "
                    "compare two builds bit for bit")
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--nbest", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mwer_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    from scattennet_amd.heads import CTCLossOp
    dev = torch.device("cuda")
    if a.ensemble:
        return on_ensemble(a, S, dev)
    a.lm = a.lm or a.ngram > 0
    if a.reference or a.lm or a.heads > 1:
        return extended(a, S, dev)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev)
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    N = a.nbest
    nb = S.ctc_decode_nbest_device(x, il, a.beam, N, collapse_repeats=False)
    ref = nb.tokens[:, min(1, N - 1)].contiguous()
    ref_len = nb.lengths[:, min(1, N - 1)].contiguous()
    R = max(int(ref_len.max()), 1)
    ref = ref[:, :R].contiguous()
    # the CTC baselines' labels: entry 0 per clip; every entry of the replicated batch
    S1 = max(int(nb.lengths[:, 0].max()), 1)
    lab1, len1 = nb.tokens[:, 0, :S1].contiguous(), nb.lengths[:, 0].contiguous()
    SN = max(int(nb.lengths.max()), 1)
    labN, lenN = nb.tokens.reshape(a.B * N, -1)[:, :SN].contiguous(), nb.lengths.reshape(-1).contiguous()
    ilN = il.repeat_interleave(N, 0)

    # Every timed op owns its leaf: a captured backward must not meet a gradient accumulator that an
    # earlier autograd graph of the same tensor left on another stream (capture rules), so
    # nothing runs a backward on the default stream before the captures, and the statistics, whose
    # graph lives on that stream, come last and on a leaf of their own.
    def leaf():
        return x.detach().clone().requires_grad_(True)

    def mwer(z=leaf()):
        z.grad = None
        S.mwer_loss(z, il, ref, ref_len, nbest=nb).backward()

    def ctc_1target(z=leaf()):
        z.grad = None
        CTCLossOp.apply(z, lab1, il, len1)[0].backward()

    def ctc_replicated(z=leaf()):
        z.grad = None
        CTCLossOp.apply(z.repeat_interleave(N, 0), labN, ilN, lenN)[0].backward()

    refN, ref_lenN = ref.repeat_interleave(N, 0).contiguous(), ref_len.repeat_interleave(N, 0).contiguous()
    hypN = nb.tokens.reshape(a.B * N, -1).contiguous()

    def wer_pairs():
        S.wer_counts(refN, ref_lenN, hypN, lenN)

    def decode_nbest():
        S.ctc_decode_nbest_device(x, il, a.beam, N, collapse_repeats=False)

    replays = {}
    for name, fn in (("mwer", mwer), ("ctc_1target", ctc_1target), ("ctc_replicated", ctc_replicated),
                     ("wer_pairs", wer_pairs), ("decode_nbest", decode_nbest)):
        replays[name] = graphed(fn)  # one eager run on a side stream, then the capture
        for _ in range(a.warmup):
            replays[name]()
    timed = alternated(replays, a.steps, a.repeats)
    stats = statistics_of(S, leaf(), il, ref, ref_len, nb)
    if a.dump:
        z = leaf()
        loss, det = S.mwer_loss(z, il, ref, ref_len, nbest=nb, posterior_scale=0.8, return_details=True)
        loss.backward()
        torch.save({"loss": loss.detach().cpu(), "dlogits": z.grad.cpu(), **{k: v.cpu() for k, v in det.items()}}, a.dump)
    res = {"workload": "MWER loss forward + backward beside the CTC loss, graph replays", "B": a.B, "T": a.T, "C": a.C,
           "beam": a.beam, "nbest": N, "steps": a.steps, "repeats": a.repeats, "unit": "us per call",
           "statistics": stats, "graph": timed}
    m = res["graph"]
    res["mwer_over_ctc_1target"] = round(m["mwer"]["median"] / m["ctc_1target"]["median"], 3)
    res["mwer_over_ctc_replicated"] = round(m["mwer"]["median"] / m["ctc_replicated"]["median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
