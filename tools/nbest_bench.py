"""Time the second pass over the CTC beam search (scattennet_amd/nbest.py) on one MI355X at the
evaluation shape of the 2014T yaml (B = 8, T/4 = 64, C = 1124): the n-best decode, the bigram
rescore, the MBR selection and the whole chain (decode, rescore, MBR, gather), beside the 1-best
beam decode of the same build at the same beam.  Two configurations: beam 5 with N = 5 (main.py's
beam) and beam 32 with N = 32 (the widest list).  Each op is timed two ways, as in
tools/decode_bench.py: eager calls (Python, allocator and launch overhead included) and replays
of a captured graph (device time of the launches only).  Both windows end in a device
synchronise; the figure is the median of --repeats windows of --steps calls, with the spread
(min, max) beside it.  Synthetic logits N(0, 4^2), full-length clips (the longest dependent
chain), a random normalised bigram table.  Needs a GPU.

Usage: python tools/nbest_bench.py [--B 8] [--T 64] [--C 1124] [--configs 5:5,32:32] [--steps 200]
                                   [--fusion] [--ngram ORDER[,ORDER]]

--fusion adds the fused search (shallow fusion, ctc_decode_fused_nbest_device) with the same table,
weight 0.5 and bonus 0.2: `fused_nbest` beside `beam_nbest`, `fused_chain` beside `chain`, the cost
per frame of both decodes (graph median / T), and what the two searches end with on these random
logits: the lists' mean count, the merge rate (1 - count / active beams), the posterior mass of
entry 0, and how often the fused list's best total exceeds the rescored unfused list's.

--ngram ORDER adds the sparse rescore (an `NGramLM` of that order, or of each order of a comma
list, `sca_nbest_rescore_ngram`) on the same lists: `rescore_ngramK` beside `rescore`,
`chain_ngramK` beside `chain`.  The model is `NGramLM.from_sequences` on every second entry of the
lists being rescored and 2000 random gloss sequences (see `ngram_model`), so the look-ups meet
stored trigrams, stored contexts and both backoff levels; `ngram` reports its entries, the bytes of
its trie against the 4 C^2 of the dense table, and the share of each look-up outcome on the lists.

The 1-best decode of another build (the parent commit's library, SCA_LIB_PATH) is timed by
tools/decode_bench.py --beam W in the same session; this tool only runs the build it imports.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.decode_bench import graphed, windows  # noqa: E402


def ngram_model(S, order, C, nb, dev, sentences=2000, length=10):
    """The benchmark's sparse model: `NGramLM.from_sequences` of `order` on every second valid entry
    of the list batch `nb` (tokens (.., N, T)) and `sentences` random sequences of `length` tokens,
    Zipf-distributed over [1, C) (seed 1).  Returns (model on `dev`, a dict of its sizes)."""
    g = torch.Generator().manual_seed(1)
    tokens, lengths = nb.tokens.reshape(-1, nb.tokens.shape[-1]).cpu(), nb.lengths.reshape(-1).cpu()
    count = nb.count.reshape(-1).cpu()
    N = nb.lengths.shape[-1]
    seqs = [tokens[i, :int(lengths[i])].tolist() for i in range(0, len(lengths), 2) if i % N < int(count[i // N])]
    p = 1.0 / torch.arange(1, C, dtype=torch.float64)
    draws = torch.multinomial(p, sentences * length, replacement=True, generator=g) + 1
    seqs += draws.reshape(sentences, length).tolist()
    lm = S.NGramLM.from_sequences(seqs, C, order, device=dev)
    uni, bi, tri = lm.num_entries
    return lm, {"order": order, "unigrams": uni, "bigrams": bi, "trigrams": tri, "trie_bytes": lm.nbytes,
                "dense_bytes": 4 * C * C, "sentences": len(seqs)}


def ngram_outcomes(lm, nb):
    """The share of each look-up outcome of `lm` over the valid entries of `nb`, on the host."""
    bi, tri = set(lm.bigram_dict()), set(lm.trigram_dict())
    tokens, lengths = nb.tokens.reshape(-1, nb.tokens.shape[-1]).cpu(), nb.lengths.reshape(-1).cpu()
    count, N = nb.count.reshape(-1).cpu(), nb.lengths.shape[-1]
    seen = dict.fromkeys(("trigram_hit", "context_hit", "context_miss", "bigram_hit", "bigram_miss"), 0)
    for i in range(len(lengths)):
        if i % N >= int(count[i // N]):
            continue
        path = [0] + tokens[i, :int(lengths[i])].tolist() + [0]
        for k in range(1, len(path)):
            if lm.order == 3 and k >= 2:
                if tuple(path[k - 2:k + 1]) in tri:
                    seen["trigram_hit"] += 1
                    continue
                seen["context_hit" if tuple(path[k - 2:k]) in bi else "context_miss"] += 1
            if lm.order >= 2:
                seen["bigram_hit" if tuple(path[k - 1:k + 1]) in bi else "bigram_miss"] += 1
    terms = max(sum(seen.values()) - seen["context_hit"] - seen["context_miss"], 1)
    return {k: round(v / terms, 4) for k, v in seen.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--configs", default="5:5,32:32", help="beam:nbest pairs")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--fusion", action="store_true", help="also time the fused search and compare its lists")
    ap.add_argument("--ngram", default="", help="also time the sparse rescore with an NGramLM of this order (or "
                    "of each order of a comma list) estimated by from_sequences")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nbest_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev)
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    lm = S.BigramLM(torch.log_softmax(torch.randn(a.C, a.C, generator=g) * 2, -1), device=dev)
    res = {"workload": "n-best CTC decode, bigram rescore, MBR", "B": a.B, "T": a.T, "C": a.C, "steps": a.steps,
           "repeats": a.repeats, "unit": "us per call: [median, min, max]", "configs": {}}
    for pair in a.configs.split(","):
        W, N = (int(v) for v in pair.split(":"))
        nb = S.ctc_decode_nbest_device(x, il, W, N)
        total, post, order = S.rescore_nbest_device(nb, lm, 0.5, 0.2)
        spec = S.Rescoring(N, lm, 0.5, 0.2, select="mbr")
        ops = {
            "beam_1best": lambda: S.ctc_decode_device(x, il, W),
            "beam_nbest": lambda: S.ctc_decode_nbest_device(x, il, W, N),
            "rescore": lambda: S.rescore_nbest_device(nb, lm, 0.5, 0.2),
            "mbr": lambda: S.mbr_select_device(nb, post),
            "chain": lambda: S.rescored_decode([x], il, W, spec),
        }
        out = {"merged_count_mean": round(float(nb.count.float().mean()), 2)}
        for k in (int(v) for v in a.ngram.split(",") if v):
            ng, sizes = ngram_model(S, k, a.C, nb, dev)
            out[f"ngram{k}"] = dict(sizes, outcomes=ngram_outcomes(ng, nb))
            ops[f"rescore_ngram{k}"] = lambda ng=ng: S.rescore_nbest_device(nb, ng, 0.5, 0.2)
            nspec = S.Rescoring(N, ng, 0.5, 0.2, select="mbr")
            ops[f"chain_ngram{k}"] = lambda nspec=nspec: S.rescored_decode([x], il, W, nspec)
        if a.fusion:
            fspec = S.Rescoring(N, lm, 0.5, 0.2, select="mbr", fusion=True)
            ops["fused_nbest"] = lambda: S.ctc_decode_fused_nbest_device(x, il, W, lm, 0.5, 0.2, N)
            ops["fused_chain"] = lambda: S.rescored_decode([x], il, W, fspec)
            fnb = ops["fused_nbest"]()
            ftotal, fpost, forder = S.rescore_nbest_device(fnb, lm, 0.5, 0.2)
            raw = S.ctc_decode_fused_nbest_device(x, il, W, lm, 0.5, 0.2, N, collapse_repeats=False).count.float()
            out["fused"] = {
                "count_mean": round(float(fnb.count.float().mean()), 2),
                "merge_rate": round(float(1 - (fnb.count.float() / raw).mean()), 4),
                "posterior_entry0_mean": round(float(fpost.gather(1, forder[:, :1].long()).mean()), 4),
                "unfused_posterior_entry0_mean": round(float(post.gather(1, order[:, :1].long()).mean()), 4),
                "best_total_gain_mean": round(float((ftotal.max(1).values - total.max(1).values).mean()), 4),
                "clips_with_larger_best_total": int((ftotal.max(1).values > total.max(1).values).sum()),
                "clips": a.B}
        for name, fn in ops.items():
            for _ in range(a.warmup):
                fn()
            out[name + "_eager"] = windows(fn, a.steps, a.repeats)
            replay = graphed(fn)
            for _ in range(a.warmup):
                replay()
            out[name + "_graph"] = windows(replay, a.steps, a.repeats)
        if a.fusion:
            for name in ("beam_nbest", "fused_nbest"):
                out[name + "_us_per_frame"] = round(out[name + "_graph"][0] / a.T, 3)
        res["configs"][f"beam{W}_n{N}"] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
