"""float64 restatements for tests/test_nbest.py and tests/test_gpu_nbest.py of the second pass
over the CTC beam search as include/scatten.h specifies it (sca_ctc_beam_decode_nbest,
sca_nbest_rescore, sca_nbest_mbr): the search of tests/decode_ref.py returning every final
beam, collapse / merge / stable sort, the bigram score with class 0 as the sentence boundary,
the posterior over the list, and loss / risk / arg-min with decode_ref.wer_single.  Also the
inputs the GPU cases share, with the tie margins test_nbest.py asserts on them.  numpy only; no
part of the package is used."""
import functools

import numpy as np

from tests import decode_ref as D

NEG_INF = -np.inf


def beam_search_all(logits, in_len, beam_width, preselect=False):
    """decode_ref.beam_search, statement for statement, returning every final beam: (beams,
    frame_gap) with beams = [(prefix tuple, total)] in slot order — descending total, ties in
    the order of the last selection — and frame_gap the smallest difference over all frames
    between the last kept and the first dropped item."""
    x = np.asarray(logits, np.float64)
    T, C = x.shape
    Tb = int(min(max(int(in_len), 0), T))
    lp_all = D.log_softmax(x)
    la = np.logaddexp
    beams = [((), 0.0, NEG_INF)]
    frame_gap = np.inf
    for t in range(Tb):
        lp = lp_all[t]
        active = {p: (i, lb, ll, la(lb, ll)) for i, (p, lb, ll) in enumerate(beams)}
        items = []
        for i, (p, lb, ll) in enumerate(beams):
            tot = la(lb, ll)
            nlb = tot + lp[0]
            nll = NEG_INF
            if p:
                e = p[-1]
                nll = ll + lp[e]
                q = p[:-1]
                if q in active:
                    _, lb_q, _, tot_q = active[q]
                    nll = la(nll, lp[e] + (lb_q if (q and e == q[-1]) else tot_q))
            items.append((la(nlb, nll), (0, i, 0), p, nlb, nll))
        cs = np.arange(1, C)
        if preselect:
            cs = cs[np.lexsort((cs, -lp[1:]))][:beam_width + 1]
        for j, (q, lb_q, ll_q) in enumerate(beams):
            tot_q = la(lb_q, ll_q)
            ll = lp[cs] + tot_q
            if q:
                ll = np.where(cs == q[-1], lp[cs] + lb_q, ll)
            children = [p[-1] for p in active if p and p[:-1] == q]
            keep = ~np.isin(cs, children) & (ll != NEG_INF)
            cq, ll = cs[keep], ll[keep]
            for n in np.lexsort((cq, -ll))[:beam_width + 1]:
                items.append((ll[n], (1, j, int(cq[n])), q + (int(cq[n]),), NEG_INF, ll[n]))
        items.sort(key=lambda it: (-it[0], it[1]))
        if len(items) > beam_width:
            frame_gap = min(frame_gap, float(items[beam_width - 1][0]) - float(items[beam_width][0]))
        beams = [(p, lb, ll) for _, _, p, lb, ll in items[:beam_width]]
    return [(p, float(la(lb, ll))) for p, lb, ll in beams], frame_gap


def adjacent_gap(values):
    """The smallest difference between neighbours of a descending sequence (inf for < 2)."""
    v = [float(a) for a in values]
    return min((a - b for a, b in zip(v[:-1], v[1:])), default=np.inf)


def merge_sort(entries, collapse_repeats):
    """[(labels, score)] in entry order -> the same after the header's collapse rule: groupby on
    every entry, equal entries merged into the first of them (logaddexp in entry order), then a
    stable sort by score, descending.  Without collapse_repeats the list is returned as it is."""
    if not collapse_repeats:
        return [(list(h), float(s)) for h, s in entries]
    merged = []
    for h, s in entries:
        h = D.collapse(list(h))
        for m in merged:
            if m[0] == h:
                m[1] = float(np.logaddexp(m[1], s))
                break
        else:
            merged.append([h, float(s)])
    merged.sort(key=lambda m: -m[1])  # list.sort is stable
    return [(h, s) for h, s in merged]


def nbest(logits, in_len, beam_width, n, collapse_repeats=True, preselect=False):
    """One clip: (entries [(labels, score)] of the n-best list, gaps): gaps = {"frame",
    "final": adjacent totals of the beams that decide the first n entries, "merged": adjacent
    scores of the merged list}."""
    beams, frame_gap = beam_search_all(logits, in_len, beam_width, preselect)
    final_gap = adjacent_gap([s for _, s in beams[:n + 1]])
    entries = merge_sort(beams[:n], collapse_repeats)
    return entries, {"frame": frame_gap, "final": final_gap, "merged": adjacent_gap([s for _, s in entries])}


def bigram_score(lm, h):
    """lm(h): class 0 is the boundary on either side; the empty hypothesis costs lm[0, 0]."""
    path = [0] + [int(v) for v in h] + [0]
    return float(sum(lm[p, c] for p, c in zip(path[:-1], path[1:])))


def rescore(entries, lm=None, lm_weight=0.0, length_bonus=0.0, posterior_scale=1.0):
    """(total, posterior, order) over the entries of one list."""
    total = np.array([s + lm_weight * (bigram_score(lm, h) if lm is not None else 0.0) + length_bonus * len(h)
                      for h, s in entries], np.float64)
    z = posterior_scale * total
    p = np.exp(z - z.max())
    order = sorted(range(len(entries)), key=lambda i: (-total[i], i))
    return total, p / p.sum(), order


def mbr(entries, posterior):
    """(loss (n, n) int64 with loss[i, j] the error count of hypothesis i against reference j,
    risk (n), best: the first minimum)."""
    n = len(entries)
    loss = np.zeros((n, n), np.int64)
    for i in range(n):
        for j in range(n):
            if i != j:
                loss[i, j] = sum(D.wer_single(entries[j][0], entries[i][0])[:3])
    risk = loss.astype(np.float64) @ np.asarray(posterior, np.float64)
    return loss, risk, int(np.argmin(risk))


def full(logits, in_lens, beam_width, n, collapse_repeats=True, lm=None, lm_weight=0.0, length_bonus=0.0,
         posterior_scale=1.0):
    """The whole chain for a batch (B, T, C): a list of per-clip dicts {entries, total, posterior,
    order, loss, risk, best, gaps}; gaps adds "total" (adjacent sorted totals) and "risk" (the two
    smallest risks)."""
    out = []
    for b in range(len(logits)):
        entries, gaps = nbest(logits[b], in_lens[b], beam_width, n, collapse_repeats)
        total, post, order = rescore(entries, lm, lm_weight, length_bonus, posterior_scale)
        loss, risk, best = mbr(entries, post)
        gaps = dict(gaps, total=adjacent_gap(total[order]), risk=adjacent_gap(-np.sort(risk)[:2]))
        out.append({"entries": entries, "total": total, "posterior": post, "order": order, "loss": loss,
                    "risk": risk, "best": best, "gaps": gaps})
    return out


def random_lm(C, seed=0):
    """A dense (C, C) table of normalised log-probabilities, float32."""
    return D.log_softmax(np.random.default_rng(1000 + seed).normal(0.0, 2.0, (C, C))).astype(np.float32)


# ------------------------------------------------------------------ the GPU cases' inputs
LM_WEIGHT, LENGTH_BONUS, POSTERIOR_SCALE = 0.6, 0.4, 0.8
# (B, T, C, W, N) -> (seed, in_len): ragged lengths with 0 and 1 (count < N)
CASES = {
    (5, 16, 4, 8, 8): (0, [16, 0, 1, 9, 16]),      # the returning-prefix case; merges are frequent
    (4, 12, 6, 8, 3): (0, [12, 0, 1, 7]),          # N < W
    (3, 20, 33, 32, 32): (0, [20, 1, 13]),         # the widest beam and list
    (2, 64, 1124, 5, 5): (0, [64, 37]),            # the evaluation shape
    # T = 128, the limit of sca_nbest_mbr: entries of 102-104 and 78-79 tokens, so the rescoring
    # wave sums more than 64 gathers and MWER's lattices have L = 205-209 and 157-159
    (2, 128, 12, 8, 8): (0, [128, 97]),
}


MODEL_BEAM = 8  # the beam of the step tests on tests/golden/model_small (nbest 3, select "mbr")


def case_logits(shape):
    B, T, C, _, _ = shape
    return np.random.default_rng(CASES[shape][0]).normal(0.0, 4.0, (B, T, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_ref(shape, collapse_repeats=True, rescored=True):
    """The restatement of one GPU case, computed once and shared: `full` with the case's table
    and weights, or (rescored=False) without table, weight and bonus."""
    _, _, C, W, N = shape
    kw = dict(lm=random_lm(C), lm_weight=LM_WEIGHT, length_bonus=LENGTH_BONUS) if rescored else {}
    return full(case_logits(shape), CASES[shape][1], W, N, collapse_repeats, posterior_scale=POSTERIOR_SCALE, **kw)
