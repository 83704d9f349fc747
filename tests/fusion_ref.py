"""float64 restatement for tests/test_fusion.py and tests/test_gpu_fusion.py of shallow fusion as
include/scatten.h specifies it (sca_ctc_beam_decode_fused_nbest): the search of
tests/nbest_ref.py with every prefix carrying the bonus g(prefix), the per-frame cut by
key = total + g, the final order by total + g + the closing bigram, and acoustic scores out.
Also the inputs the CPU and GPU cases share.  numpy only; no part of the package is used."""
import functools

import numpy as np

from tests import decode_ref as D
from tests import nbest_ref as R

NEG_INF = -np.inf
PRESELECT = (None, "per_beam", "shared")


def search(logits, in_len, beam_width, lm=None, lm_weight=0.0, length_bonus=0.0, preselect=None, dtype=np.float64):
    """One clip, logits (T, C): (beams, frame_gap, final_gap).  beams = [(prefix tuple, total,
    final key)] in the final order (final key descending, ties to the lower slot); frame_gap the
    smallest key difference over all frames between the last kept and the first dropped item,
    final_gap the smallest difference between adjacent final keys.
    preselect: None — every label is a candidate of every beam; "per_beam" — a beam's candidates
    come from the beam_width + 1 labels with the largest lp[c] + lm_weight * lm[last, c] (ties to
    the lower class), as the kernel does; "shared" — from the frame's beam_width + 1 labels with
    the largest lp[c], the unfused kernel's list, which is NOT exact here.
    dtype: the arithmetic's float type."""
    if preselect not in PRESELECT:
        raise ValueError(f"preselect must be one of {PRESELECT}")
    x = np.asarray(logits, np.float64)
    T, C = x.shape
    Tb = int(min(max(int(in_len), 0), T))
    lp_all = D.log_softmax(x).astype(dtype)
    table = np.zeros((C, C), dtype) if lm is None else np.asarray(lm).astype(dtype)
    w, bonus = dtype(lm_weight), dtype(length_bonus)
    la = np.logaddexp
    beams = [((), dtype(0.0), dtype(NEG_INF), dtype(0.0))]  # (prefix, lb, ll, g) in slot order
    frame_gap = np.inf
    for t in range(Tb):
        lp = lp_all[t]
        active = {p: (i, lb, ll, la(lb, ll)) for i, (p, lb, ll, _) in enumerate(beams)}
        items = []  # (key, order key, prefix, lb, ll, g)
        for i, (p, lb, ll, g) in enumerate(beams):
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
            items.append((la(nlb, nll) + g, (0, i, 0), p, nlb, nll, g))
        shared = np.arange(1, C)
        shared = shared[np.lexsort((shared, -lp[1:]))][:beam_width + 1]
        for j, (q, lb_q, ll_q, g_q) in enumerate(beams):
            tot_q = la(lb_q, ll_q)
            last = q[-1] if q else 0
            cs = np.arange(1, C)
            if preselect == "per_beam":
                cs = cs[np.lexsort((cs, -(lp[1:] + w * table[last, 1:])))][:beam_width + 1]
            elif preselect == "shared":
                cs = shared
            ll = lp[cs] + tot_q
            if q:
                ll = np.where(cs == last, lp[cs] + lb_q, ll)
            g = g_q + w * table[last, cs] + bonus
            children = [p[-1] for p in active if p and p[:-1] == q]
            keep = ~np.isin(cs, children) & (ll != NEG_INF)
            cq, ll, g = cs[keep], ll[keep], g[keep]
            key = ll + g
            for n in np.lexsort((cq, -key))[:beam_width + 1]:
                items.append((key[n], (1, j, int(cq[n])), q + (int(cq[n]),), dtype(NEG_INF), ll[n], g[n]))
        items.sort(key=lambda it: (-it[0], it[1]))
        if len(items) > beam_width:
            frame_gap = min(frame_gap, float(items[beam_width - 1][0]) - float(items[beam_width][0]))
        beams = [(p, lb, ll, g) for _, _, p, lb, ll, g in items[:beam_width]]
    final = [(p, la(lb, ll), la(lb, ll) + g + w * table[p[-1] if p else 0, 0]) for p, lb, ll, g in beams]
    final.sort(key=lambda b: -b[2])  # stable: ties to the lower slot
    final = [(p, float(tot), float(key)) for p, tot, key in final]
    return final, frame_gap, R.adjacent_gap([k for _, _, k in final])


def fused_nbest(logits, in_len, beam_width, n, collapse_repeats=True, lm=None, lm_weight=0.0, length_bonus=0.0,
                preselect=None, dtype=np.float64):
    """One clip: (entries [(labels, acoustic score)] of the fused n-best list, keys: the final keys
    of the beams behind the first n uncollapsed entries, gaps {"frame", "final", "merged"})."""
    beams, frame_gap, _ = search(logits, in_len, beam_width, lm, lm_weight, length_bonus, preselect, dtype)
    final_gap = R.adjacent_gap([k for _, _, k in beams[:n + 1]])
    entries = R.merge_sort([(p, s) for p, s, _ in beams[:n]], collapse_repeats)
    gaps = {"frame": frame_gap, "final": final_gap, "merged": R.adjacent_gap([s for _, s in entries])}
    return entries, [k for _, _, k in beams[:n]], gaps


def full(logits, in_lens, beam_width, n, collapse_repeats=True, lm=None, lm_weight=0.0, length_bonus=0.0,
         posterior_scale=1.0, dtype=np.float64):
    """The whole chain for a batch (B, T, C) — fused list, rescore with the same table, weight and
    bonus, MBR — as nbest_ref.full returns it, plus "keys"."""
    out = []
    for b in range(len(logits)):
        entries, keys, gaps = fused_nbest(logits[b], in_lens[b], beam_width, n, collapse_repeats, lm, lm_weight,
                                          length_bonus, "per_beam", dtype)
        total, post, order = R.rescore(entries, lm, lm_weight, length_bonus, posterior_scale)
        loss, risk, best = R.mbr(entries, post)
        gaps = dict(gaps, total=R.adjacent_gap(total[order]), risk=R.adjacent_gap(-np.sort(risk)[:2]))
        out.append({"entries": entries, "keys": keys, "total": total, "posterior": post, "order": order,
                    "loss": loss, "risk": risk, "best": best, "gaps": gaps})
    return out


# ------------------------------------------------------------------ the shared cases' inputs
BONUS = 0.2
WEIGHTS = (0.5, 3.0)
POSTERIOR_SCALE = 0.8
# (B, T, C, W, N) -> (seed, in_len): ragged lengths with 0 and 1; (5, 16, 4, 8, 8) has C - 1 < W + 1
CASES = {
    (5, 16, 4, 8, 8): (0, [16, 0, 1, 9, 16]),
    (4, 12, 6, 8, 3): (0, [12, 0, 1, 7]),
    (3, 20, 33, 32, 32): (0, [20, 1, 13]),
    (2, 64, 1124, 5, 5): (0, [64, 37]),
    (2, 128, 12, 8, 8): (0, [128, 97]),  # nbest_ref's long case: entries of more than 64 tokens
}


def case_logits(shape):
    B, T, C, _, _ = shape
    return np.random.default_rng(CASES[shape][0]).normal(0.0, 4.0, (B, T, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case_ref(shape, lm_weight, collapse_repeats=True, dtype=np.float64):
    """The restatement of one GPU case, computed once and shared."""
    _, _, C, W, N = shape
    return full(case_logits(shape), CASES[shape][1], W, N, collapse_repeats, R.random_lm(C), lm_weight, BONUS,
                POSTERIOR_SCALE, dtype)


def constructed_case():
    """(logits (1, 3, 12), lm (12, 12), lm_weight, W): beam width 2.  Frame 0 makes (1) the best
    beam.  At frame 1 labels 1, 2 and 3 are the frame's top-(W + 1) by lp and label 9 is far down
    the list, but lm[1, 9] is the only bigram after 1 that is not heavily penalised: with the
    table, (1, 9) enters the beam, which the frame-wide list cannot produce."""
    C = 12
    x = np.full((1, 3, C), -6.0, np.float32)
    x[0, 0, 1], x[0, 0, 2], x[0, 0, 0] = 4.0, 1.5, 0.0
    x[0, 1, 1], x[0, 1, 2], x[0, 1, 3], x[0, 1, 9], x[0, 1, 0] = 2.0, 1.7, 1.3, -1.0, -3.0
    x[0, 2, 0], x[0, 2, 4] = 3.0, 0.3  # frame 2 cannot bring label 9 in
    x += np.random.default_rng(5).normal(0.0, 0.05, x.shape).astype(np.float32)
    lm = np.full((C, C), -3.0, np.float32)
    lm[1, :] = -9.0
    lm[1, 9] = -0.2
    lm[1, 0] = -1.0
    lm += np.random.default_rng(6).normal(0.0, 0.05, lm.shape).astype(np.float32)
    return x, lm, 1.0, 2


FALLBACK_SHAPE = (1, 3, 1124, 16, 16)  # (B, T, C, W, N)
FALLBACK_LIST = 256                    # DEC_FUSE_LIST of csrc/decode.hip


def fallback_case():
    """(logits (1, 3, 1124), lm, lm_weight, bonus): every label of 16 of the kernel's 64 lanes
    (label c belongs to lane (c - 1) % 64) is large, a 17th lane's best is in the middle and the
    rest are small, so the threshold of the per-beam selection (the (W + 1)-th largest lane
    maximum) lets 16 * 18 labels through: more than the list holds, which takes the kernel's
    round-by-round path."""
    _, T, C, _, _ = FALLBACK_SHAPE
    rng = np.random.default_rng(2)
    x = rng.uniform(0.0, 1.0, (1, T, C)).astype(np.float32)
    c = np.arange(C)
    big = (c >= 1) & ((c - 1) % 64 < 16)
    x[:, :, big] = rng.uniform(9.0, 15.0, (1, T, int(big.sum()))).astype(np.float32)
    x[:, :, 17] = 5.0  # lane 16
    return x, R.random_lm(C), 0.3, BONUS


def labels_over_threshold(lp_row, lm_row, lm_weight, k):
    """How many labels reach the k-th largest of the 64 lanes' maxima of lp + lm_weight * lm."""
    key = np.asarray(lp_row, np.float64)[1:] + lm_weight * np.asarray(lm_row, np.float64)[1:]
    lane_max = [key[lane::64].max() for lane in range(min(64, len(key)))]
    return int((key >= sorted(lane_max, reverse=True)[k - 1]).sum())


def wins_case():
    """(logits (1, 10, 9), lm (9, 9), lm_weight, bonus, W): a seeded case in which the fused search
    ends with a strictly larger best total than the rescored unfused list of the same width."""
    rng = np.random.default_rng(1)
    x = rng.normal(0.0, 1.5, (1, 10, 9)).astype(np.float32)
    lm = D.log_softmax(rng.normal(0.0, 3.0, (9, 9))).astype(np.float32)
    return x, lm, 2.0, 0.0, 3
