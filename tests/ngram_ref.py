"""float64 restatement for tests/test_ngram.py and tests/test_gpu_ngram.py of the backoff n-gram
gloss model as include/scatten.h specifies it (sca_ngram_lm, sca_nbest_rescore_ngram,
sca_mwer_heads_fwd_ngram): the score of a labelling through plain dicts with the ARPA backoff
rule and the header's order of additions, random sparse tables, and the GPU cases' inputs with
the tie margins and look-up outcomes test_ngram.py asserts on them.  The lists, `rescore`, `mbr`,
`CASES` and the weights are those of tests/nbest_ref.py.  numpy only; no part of the package is
used.

A model here is a dict: order, C, uni_lp, uni_bo (C) float32 arrays, bi {(v, w): (lp, bo)} and
tri {(u, v, w): lp} with float32-representable values."""
import functools

import numpy as np

from tests import decode_ref as D
from tests import nbest_ref as R

OUTCOMES = ("trigram hit", "context hit", "context miss", "bigram hit", "bigram miss")
# the GPU cases: the shapes of nbest_ref.CASES the n-gram tests run, and their table's seed
SHAPES = [(5, 16, 4, 8, 8), (3, 20, 33, 32, 32), (2, 128, 12, 8, 8), (2, 64, 1124, 5, 5)]
SEED = 0
DENSE_ROWS = 1 << 21  # trigram cells above which only some contexts get a row (random_ngram)
EXTRA_CONTEXTS = 1024


def p2(model, v, w, seen=None):
    """p2(w | v) = bi_lp[v, w] if stored, else uni_bo[v] + uni_lp[w]."""
    hit = (v, w) in model["bi"]
    if seen is not None:
        seen["bigram hit" if hit else "bigram miss"] += 1
    return float(model["bi"][v, w][0]) if hit else float(model["uni_bo"][v]) + float(model["uni_lp"][w])


def p3(model, u, v, w, seen=None):
    """p3(w | u, v) = tri_lp[u, v, w] if stored; else bi_bo[u, v] + p2(w | v) if (u, v) is a stored
    bigram; else p2(w | v)."""
    if (u, v, w) in model["tri"]:
        if seen is not None:
            seen["trigram hit"] += 1
        return float(model["tri"][u, v, w])
    ctx = (u, v) in model["bi"]
    if seen is not None:
        seen["context hit" if ctx else "context miss"] += 1
    back = p2(model, v, w, seen)
    return float(model["bi"][u, v][1]) + back if ctx else back


def terms(model, h, seen=None):
    """The len + 1 terms of lm(h): path = [0] + h + [0]; the term at k uses two previous elements
    with order 3 and k >= 2, one at k = 1 and with order 2, none with order 1."""
    path = [0] + [int(t) for t in h] + [0]
    out = []
    for k in range(1, len(path)):
        if model["order"] == 1:
            out.append(float(model["uni_lp"][path[k]]))
        elif model["order"] == 2 or k == 1:
            out.append(p2(model, path[k - 1], path[k], seen))
        else:
            out.append(p3(model, path[k - 2], path[k - 1], path[k], seen))
    return out


def score(model, h, seen=None):
    """lm(h); `seen`: a dict over OUTCOMES that counts the look-ups' outcomes."""
    return float(sum(terms(model, h, seen)))


def prior(model, h, lm_weight, length_bonus, seen=None):
    return lm_weight * (score(model, h, seen) if model is not None else 0.0) + length_bonus * len(h)


def truncated(model, order):
    """The model with the n-grams above `order` dropped."""
    return dict(model, order=order, bi=model["bi"] if order >= 2 else {}, tri=model["tri"] if order >= 3 else {})


def support_contexts(support):
    """The trigram contexts (path[k-2], path[k-1]), k >= 2, of the labellings in `support`."""
    out = set()
    for h in support:
        path = [0] + [int(t) for t in h] + [0]
        out.update(zip(path[:-2], path[1:-1]))
    return out


def random_ngram(C, order, seed=0, support=()):
    """A sparse random model: about half of the (C, C) bigram cells are stored, and about 0.4 of
    the cells of the trigram rows.  Every stored bigram (u, v), v != 0, is a trigram context while
    that gives at most DENSE_ROWS cells; above it (the evaluation vocabulary) the contexts are
    those of the labellings in `support` that are stored bigrams and EXTRA_CONTEXTS others, so
    that a list over a thousand classes meets stored trigrams at all.  Whether a cell is stored
    and its value depend on (seed, cell) alone, never on `support`.  Values are float32: rows of
    log-softmaxes for the probabilities, small negative numbers for the backoff weights."""
    rng = np.random.default_rng(2000 + seed)
    f32 = np.float32
    model = {"order": order, "C": C, "uni_lp": D.log_softmax(rng.normal(0.0, 2.0, C)).astype(f32),
             "uni_bo": (-np.abs(rng.normal(0.0, 0.5, C))).astype(f32), "bi": {}, "tri": {}}
    if order >= 2:
        keep = rng.random((C, C)) < 0.5
        lp = D.log_softmax(rng.normal(0.0, 2.0, (C, C))).astype(f32)
        bo = (-np.abs(rng.normal(0.0, 0.5, (C, C)))).astype(f32)
        vs, ws = np.nonzero(keep)
        model["bi"] = {(int(v), int(w)): (lp[v, w], bo[v, w]) for v, w in zip(vs, ws)}
    if order >= 3:
        contexts = [(int(u), int(v)) for u, v in zip(vs, ws) if v != 0]
        if len(contexts) * C > DENSE_ROWS:
            wanted = support_contexts(support)
            extra = np.random.default_rng(3000 + seed).permutation(len(contexts))[:EXTRA_CONTEXTS]
            contexts = sorted({c for c in contexts if c in wanted} | {contexts[i] for i in extra})
        for u, v in contexts:
            row = np.random.default_rng([4000 + seed, u, v])
            stored = np.nonzero(row.random(C) < 0.4)[0]
            vals = D.log_softmax(row.normal(0.0, 2.0, C)).astype(f32)
            for w in stored:
                model["tri"][u, v, int(w)] = vals[w]
    return model


# ------------------------------------------------------------------ the GPU cases' inputs
def case_entries(shape):
    """The collapsed lists of one case: per clip [(labels, score)], nbest_ref's."""
    return [clip["entries"] for clip in R.case_ref(shape)]


@functools.lru_cache(maxsize=None)
def case_model(shape, order=3):
    """The case's table: one order-3 draw per shape, truncated for the lower orders."""
    if order < 3:
        return truncated(case_model(shape), order)
    support = [h for entries in case_entries(shape) for h, _ in entries]
    return random_ngram(shape[2], 3, SEED, support)


def chain(entries, model, lm_weight, length_bonus, posterior_scale, seen=None):
    """nbest_ref's rescore and mbr over one list with the n-gram prior inside the totals:
    {total, posterior, order, loss, risk, best, gaps}."""
    primed = [(h, s + prior(model, h, lm_weight, length_bonus, seen)) for h, s in entries]
    total, post, order = R.rescore(primed, posterior_scale=posterior_scale)
    loss, risk, best = R.mbr(entries, post)
    gaps = {"total": R.adjacent_gap(total[order]), "risk": R.adjacent_gap(-np.sort(risk)[:2])}
    return {"entries": entries, "total": total, "posterior": post, "order": order, "loss": loss, "risk": risk,
            "best": best, "gaps": gaps}


@functools.lru_cache(maxsize=None)
def case_ref(shape, order=3):
    """The restatement of one GPU case, computed once and shared: (clips, seen) with the chain of
    every clip under the case's weights and the outcome counts of all its look-ups."""
    seen = dict.fromkeys(OUTCOMES, 0)
    model = case_model(shape, order)
    clips = [chain(entries, model, R.LM_WEIGHT, R.LENGTH_BONUS, R.POSTERIOR_SCALE, seen)
             for entries in case_entries(shape)]
    return clips, seen


def build(cls, model, device=None):
    """The model as the package's class `cls` (scattennet_amd.NGramLM), for the tests."""
    return cls(model["order"], model["C"], model["uni_lp"], model["uni_bo"], model["bi"] or None,
               model["tri"] or None, device=device)
