"""float64 restatements for tests/test_decode.py: the CTC prefix beam search as
include/scatten.h specifies it (word for word, prefixes as tuples), the best-path decoder, the
exhaustive enumeration over all C^T paths, and metrics.wer_single / wer_list
(metrics.py:2754-2907) on token-id sequences.  numpy only; no part of the package is used."""
import itertools

import numpy as np

NEG_INF = -np.inf
WER_COST_DEL, WER_COST_INS, WER_COST_SUB = 3, 3, 4


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def collapse(seq):
    """utils.py:185-188: [x[0] for x in groupby(seq)]"""
    return [k for k, _ in itertools.groupby(seq)]


def beam_search(logits, in_len, beam_width, collapse_repeats=False, preselect=False, dtype=np.float64):
    """One clip: logits (T, C).  Returns (labels, score, frame_gap, final_gap): frame_gap is the
    smallest difference over all frames between the last kept and the first dropped candidate's
    total, final_gap the difference between the best and the second final beam (inf where
    there is no such pair).  preselect: candidates only from the beam_width + 1 labels with the
    largest lp (ties to the lower class), as the kernel does.  dtype: the arithmetic's float
    type (float32 to see what rounding does to a case)."""
    x = np.asarray(logits, np.float64)
    T, C = x.shape
    Tb = int(min(max(int(in_len), 0), T))
    lp_all = log_softmax(x).astype(dtype)
    la = np.logaddexp
    # beams: list of (prefix tuple, lb, ll) in slot order
    beams = [((), dtype(0.0), dtype(NEG_INF))]
    frame_gap = np.inf
    for t in range(Tb):
        lp = lp_all[t]
        active = {p: (i, lb, ll, la(lb, ll)) for i, (p, lb, ll) in enumerate(beams)}
        items = []  # (total, order key, prefix, lb, ll)
        for i, (p, lb, ll) in enumerate(beams):
            tot = la(lb, ll)
            nlb = tot + lp[0]
            nll = dtype(NEG_INF)
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
            # only a beam's beam_width + 1 best candidates (in the order of the final sort) can
            # be among the first beam_width + 1 items, which is all that is read below
            for n in np.lexsort((cq, -ll))[:beam_width + 1]:
                items.append((ll[n], (1, j, int(cq[n])), q + (int(cq[n]),), dtype(NEG_INF), ll[n]))
        items.sort(key=lambda it: (-it[0], it[1]))
        if len(items) > beam_width:
            frame_gap = min(frame_gap, float(items[beam_width - 1][0]) - float(items[beam_width][0]))
        beams = [(p, lb, ll) for _, _, p, lb, ll in items[:beam_width]]
    totals = [la(lb, ll) for _, lb, ll in beams]
    best = int(np.argmax(totals))  # the first maximum: ties to the lower slot
    rest = [float(v) for i, v in enumerate(totals) if i != best]
    final_gap = float(totals[best]) - max(rest) if rest else np.inf
    labels = list(beams[best][0])
    if collapse_repeats:
        labels = collapse(labels)
    return labels, float(totals[best]), frame_gap, final_gap


def beam_search_batch(logits, in_len, beam_width, collapse_repeats=False, **kw):
    """logits (B, T, C) -> (list of label lists, scores (B,), smallest frame gap, smallest final gap)"""
    out = [beam_search(logits[b], in_len[b], beam_width, collapse_repeats, **kw) for b in range(len(logits))]
    return ([o[0] for o in out], np.array([o[1] for o in out]), min(o[2] for o in out), min(o[3] for o in out))


def greedy(logits, in_len):
    """Best path of one clip: (labels, score)."""
    x = np.asarray(logits, np.float64)
    Tb = int(min(max(int(in_len), 0), x.shape[0]))
    lp = log_softmax(x[:Tb])
    path = lp.argmax(-1) if Tb else np.zeros(0, np.int64)  # the first maximum: ties to the lower class
    labels = [int(c) for c in collapse(path.tolist()) if c != 0]
    return labels, float(lp[np.arange(Tb), path].sum()) if Tb else 0.0


def exhaustive(logits):
    """All C^T paths of one clip (T, C): {labelling: log-probability}, the labelling being the
    path with repeats merged and blanks removed."""
    lp = log_softmax(logits)
    T, C = lp.shape
    acc = {}
    for path in itertools.product(range(C), repeat=T):
        lab = tuple(c for c in collapse(path) if c != 0)
        acc[lab] = np.logaddexp(acc.get(lab, NEG_INF), sum(lp[t, c] for t, c in enumerate(path)))
    return acc


# ---------------------------------------------------------------------- metrics.py:2793-2907
def edit_distance(r, h):
    """metrics.edit_distance with int64 cells (the reference's uint8 wraps above 255)."""
    d = np.zeros((len(r) + 1, len(h) + 1), np.int64)
    d[0, :] = np.arange(len(h) + 1) * WER_COST_INS
    d[:, 0] = np.arange(len(r) + 1) * WER_COST_DEL
    for i in range(1, len(r) + 1):
        for j in range(1, len(h) + 1):
            if r[i - 1] == h[j - 1]:
                d[i, j] = d[i - 1, j - 1]
            else:
                d[i, j] = min(d[i - 1, j - 1] + WER_COST_SUB, d[i, j - 1] + WER_COST_INS, d[i - 1, j] + WER_COST_DEL)
    return d


def alignment(r, h, d):
    """metrics.get_alignment's list of steps, statement by statement (without the printout)."""
    x, y = len(r), len(h)
    max_len = 3 * (x + y)
    steps = []
    while True:
        if (x <= 0 and y <= 0) or (len(steps) > max_len):
            break
        elif x >= 1 and y >= 1 and d[x][y] == d[x - 1][y - 1] and r[x - 1] == h[y - 1]:
            steps.append("C")
            x, y = max(x - 1, 0), max(y - 1, 0)
        elif x >= 1 and y >= 1 and d[x][y] == d[x - 1][y - 1] + WER_COST_SUB:
            steps.append("S")
            x, y = max(x - 1, 0), max(y - 1, 0)
        elif y >= 1 and d[x][y] == d[x][y - 1] + WER_COST_INS:
            steps.append("I")
            y = max(y - 1, 0)
        else:
            steps.append("D")
            x = max(x - 1, 0)
    return steps[::-1]


def wer_single(r, h):
    """(num_del, num_ins, num_sub, num_ref) of metrics.wer_single for two token sequences."""
    r, h = list(r), list(h)
    a = alignment(r, h, edit_distance(r, h))
    return a.count("D"), a.count("I"), a.count("S"), len(r)


def wer_list(refs, hyps):
    """metrics.wer_list over token sequences."""
    c = np.array([wer_single(r, h) for r, h in zip(refs, hyps)], np.int64).reshape(-1, 4).sum(0)
    n_del, n_ins, n_sub, n_ref = (int(v) for v in c)
    n_err = n_del + n_ins + n_sub
    n_ref, n_err, n_del, n_ins, n_sub = [v if v != 0 else 1 for v in (n_ref, n_err, n_del, n_ins, n_sub)]
    return {"wer": (n_err / n_ref) * 100, "del_rate": (n_del / n_ref) * 100, "ins_rate": (n_ins / n_ref) * 100,
            "sub_rate": (n_sub / n_ref) * 100}
