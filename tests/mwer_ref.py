"""float64 restatement for tests/test_mwer*.py and tests/test_gpu_mwer*.py of the MWER loss as
include/scatten.h specifies it (sca_mwer_fwd / sca_mwer_bwd and, with the
clip's reference as one more slot and the bigram gloss model and the length bonus inside the
posterior, sca_mwer_heads_fwd / sca_mwer_heads_bwd; a grouped call is this restatement once per
head): exact CTC log-likelihoods of the slots from torch's CPU ctc_loss (the third-party op the
project's CTC oracle rests on), the posterior over the valid slots, error counts from
decode_ref.wer_single, the centred expected error, and the gradient by torch.autograd.
`analytic_grad` restates the header's closed form (alpha / beta occupancies, clamp gate,
log-softmax backward) in numpy so that the two can be compared.  Also the inputs the GPU cases
share: the uncollapsed lists of tests/nbest_ref.py with a reference taken from each clip's own
list (`case_inputs`) or one near it that the list need not hold (`case_inputs_ext`).  No part of
the package is used."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import decode_ref as D
from tests import nbest_ref as NR

NEG_INF = -np.inf
POSTERIOR_SCALE = 0.8  # the GPU cases'
LM_WEIGHT, LENGTH_BONUS = 0.7, 0.3


def log_probs(logits):
    """clamp(log_softmax(logits), -100, 0), the log-probabilities of compute_loss (torch, float64)."""
    return torch.clamp(torch.log_softmax(logits.double(), -1), -100.0, 0.0)


def fits(h, Tb):
    """A labelling has a path of Tb frames: len + adjacent repeats <= Tb."""
    return len(h) + sum(a == b for a, b in zip(h[:-1], h[1:])) <= Tb


def loglik(lp, Tb, h):
    """The exact CTC log-likelihood of labelling h over the frames [0, Tb) of lp (T, C) as a
    differentiable 0-dim tensor, or None when h does not fit."""
    h = [int(v) for v in h]
    if not fits(h, Tb):
        return None
    if not h:
        return lp[:Tb, 0].sum()
    nll = F.ctc_loss(lp[:Tb].unsqueeze(1), torch.tensor([h]), torch.tensor([Tb]), torch.tensor([len(h)]), blank=0,
                     reduction="sum", zero_infinity=False)
    return -nll


def clip_stats(lls, errs, posterior_scale):
    """(post, risk, loss_b) of one clip from the valid entries' likelihoods (a tensor) and error
    counts; post is a tensor, so loss_b stays differentiable."""
    err = torch.tensor(errs, dtype=torch.float64)
    post = torch.softmax(posterior_scale * lls, 0)
    d = err - err.mean()
    return post, (post * err).sum(), (post * d).sum()


def prior(h, lm, lm_weight, length_bonus):
    """lmterm = lm_weight * lm(h) + length_bonus * len(h); lm = None means lm(h) = 0."""
    return lm_weight * (NR.bigram_score(lm, h) if lm is not None else 0.0) + length_bonus * len(h)


def slots(Tb, entries, ref, with_ref):
    """The slots of one clip: (labels [M], errors [M], ref_valid).  Slot N, the reference, is there
    with `with_ref`; it is valid iff it fits and no entry of the list has error count 0."""
    labels = [[int(v) for v in h] for h in entries]
    errs = [sum(D.wer_single(list(ref), h)[:3]) for h in labels]
    if not with_ref:
        return labels, errs, False
    ok = fits([int(v) for v in ref], Tb) and 0 not in errs
    return labels + [[int(v) for v in ref]], errs + [0], ok


def mwer(logits, in_lens, lists, refs, posterior_scale=1.0, n_max=None, with_ref=False, lm=None, lm_weight=0.0,
         length_bonus=0.0, grad=True):
    """One head's loss: logits (B, T, C); lists[b] the entries (label lists) of clip b, in list
    order; refs[b] the reference labels; M = n_max (default: the longest list) + with_ref slots
    per clip.  Returns a dict of float64 numpy arrays: loglik (B, M) (-inf for slots that do not
    fit or do not exist; loglik[b, N] is the reference's whenever it fits, also where the slot is
    a duplicate), posterior (B, M), errors (B, M) (int64, 0 for entries that do not exist and
    for the reference), ref_valid (B) int64, risk (B), loss, and with `grad` dlogits (B, T, C) =
    d loss / d logits by autograd."""
    x = torch.tensor(np.asarray(logits), dtype=torch.float64, requires_grad=True)
    B, T, _ = x.shape
    N = n_max or max(len(l) for l in lists)
    Ms = N + (1 if with_ref else 0)
    lp = log_probs(x)
    out = {"loglik": np.full((B, Ms), NEG_INF), "posterior": np.zeros((B, Ms)), "errors": np.zeros((B, Ms), np.int64),
           "risk": np.zeros(B), "ref_valid": np.zeros(B, np.int64)}
    loss = x.new_zeros(())
    for b in range(B):
        Tb = int(min(max(int(in_lens[b]), 0), T))
        labels, errs, ref_ok = slots(Tb, lists[b], refs[b], with_ref)
        out["ref_valid"][b] = int(ref_ok)
        valid, zs = [], []
        for k, h in enumerate(labels):
            is_ref = with_ref and k == len(labels) - 1
            n = N if is_ref else k
            out["errors"][b, n] = errs[k]
            ll = loglik(lp[b], Tb, h)
            if ll is None:
                continue
            out["loglik"][b, n] = float(ll.detach())
            if is_ref and not ref_ok:
                continue
            valid.append(n)
            zs.append(ll + prior(h, lm, lm_weight, length_bonus))
        if not valid:
            continue
        post, risk, loss_b = clip_stats(torch.stack(zs), [out["errors"][b, n] for n in valid], posterior_scale)
        out["posterior"][b, valid] = post.detach().numpy()
        out["risk"][b] = float(risk.detach())
        loss = loss + loss_b / B
    out["loss"] = float(loss.detach())
    if grad:
        out["dlogits"] = torch.autograd.grad(loss, x)[0].numpy() if loss.requires_grad else np.zeros(x.shape)
    return out


# ------------------------------------------------------------------------ the closed form
def alpha_beta(lp, Tb, h):
    """(alpha, beta) (Tb, 2 len + 1) in log space over numpy float64 lp (T, C), torch's
    convention: both include lp[t, label(s)]."""
    ext = [0]
    for c in h:
        ext += [int(c), 0]
    L = len(ext)
    la = np.logaddexp
    alpha, beta = np.full((Tb, L), NEG_INF), np.full((Tb, L), NEG_INF)
    for s in range(min(L, 2)):
        alpha[0, s] = lp[0, ext[s]]
    for s in range(max(L - 2, 0), L):
        beta[Tb - 1, s] = lp[Tb - 1, ext[s]]
    for t in range(1, Tb):
        for s in range(L):
            a = alpha[t - 1, s]
            if s >= 1:
                a = la(a, alpha[t - 1, s - 1])
            if s >= 2 and ext[s] != 0 and ext[s] != ext[s - 2]:
                a = la(a, alpha[t - 1, s - 2])
            alpha[t, s] = a + lp[t, ext[s]]
    for t in range(Tb - 2, -1, -1):
        for s in range(L):
            a = beta[t + 1, s]
            if s + 1 < L:
                a = la(a, beta[t + 1, s + 1])
            if s + 2 < L and ext[s] != 0 and ext[s] != ext[s + 2]:
                a = la(a, beta[t + 1, s + 2])
            beta[t, s] = a + lp[t, ext[s]]
    return alpha, beta, ext


def analytic_grad(logits, in_lens, lists, refs, posterior_scale=1.0, with_ref=False, lm=None, lm_weight=0.0,
                  length_bonus=0.0, dloss=1.0):
    """d loss / d logits by the header's closed form over the enlarged list, numpy float64: the
    prior is a constant of the posterior, and the reference's occupancies come from its own
    lattice."""
    x = np.asarray(logits, np.float64)
    B, T, C = x.shape
    raw = D.log_softmax(x)
    lp = np.clip(raw, -100.0, 0.0)
    gate = (raw >= -100.0) & (raw <= 0.0)
    dx = np.zeros_like(x)
    for b in range(B):
        Tb = int(min(max(int(in_lens[b]), 0), T))
        labels, errs, ref_ok = slots(Tb, lists[b], refs[b], with_ref)
        if with_ref and not ref_ok:
            labels, errs = labels[:-1], errs[:-1]
        keep = [k for k, h in enumerate(labels) if fits(h, Tb)]
        if len(keep) < 2 or Tb == 0:
            continue
        ent = [labels[k] for k in keep]
        err = np.array([errs[k] for k in keep], np.float64)
        ab = [alpha_beta(lp[b], Tb, h) for h in ent]
        ll = np.array([np.logaddexp(a[Tb - 1, -1], a[Tb - 1, -2] if a.shape[1] > 1 else NEG_INF) for a, _, _ in ab])
        z = posterior_scale * (ll + np.array([prior(h, lm, lm_weight, length_bonus) for h in ent]))
        post = np.exp(z - z.max())
        post /= post.sum()
        d = err - err.mean()
        w = dloss / B * posterior_scale * post * (d - (post * d).sum())
        g = np.zeros((Tb, C))
        for wn, lln, (alpha, beta, ext) in zip(w, ll, ab):
            for s, c in enumerate(ext):
                g[:, c] += wn * np.exp(alpha[:, s] + beta[:, s] - lp[b, :Tb, c] - lln)
        g = np.where(gate[b, :Tb], g, 0.0)
        dx[b, :Tb] = g - np.exp(raw[b, :Tb]) * g.sum(-1, keepdims=True)
    return dx


# ------------------------------------------------------------------ the GPU cases' inputs
def pick_refs(lists):
    """The reference of clip b: entry (b + 1) mod count of its own list, or [1] if that entry is
    empty — a reference near the list, so that the error counts differ within it."""
    refs = []
    for b, entries in enumerate(lists):
        h = list(entries[(b + 1) % len(entries)])
        refs.append(h if h else [1])
    return refs


@functools.lru_cache(maxsize=None)
def case_inputs(shape):
    """(logits (B, T, C) float32, in_len, lists, refs) of one nbest_ref.CASES shape: the
    restatement's uncollapsed lists."""
    clips = NR.case_ref(shape, collapse_repeats=False, rescored=False)
    lists = [[list(h) for h, _ in c["entries"]] for c in clips]
    return NR.case_logits(shape), list(NR.CASES[shape][1]), lists, pick_refs(lists)


@functools.lru_cache(maxsize=None)
def case_ref(shape):
    """The restatement of one GPU case, computed once and shared."""
    logits, in_len, lists, refs = case_inputs(shape)
    return mwer(logits, in_len, lists, refs, POSTERIOR_SCALE, n_max=shape[4])


def pick_refs_ext(lists, C):
    """The reference of clip b, from entry (b + 1) mod count of its own list.  b mod 3 == 2: that
    entry itself, the duplicate case ([1] for an empty entry).  Otherwise [1] for an empty entry,
    else the entry with h[i], i = len // 2, replaced by the smallest class in [1, C) that differs
    from h[i - 1], h[i] and h[i + 1]; if there is none, h[i] is deleted.  Neither change adds an
    adjacent repeat or a token, so len + repeats <= in_len still holds."""
    refs = []
    for b, entries in enumerate(lists):
        h = [int(v) for v in entries[(b + 1) % len(entries)]]
        if not h:
            h = [1]
        elif b % 3 != 2:
            i = len(h) // 2
            near = set(h[max(i - 1, 0):i + 2])
            free = [c for c in range(1, C) if c not in near]
            h = h[:i] + free[:1] + h[i + 1:]
        refs.append(h)
    return refs


def random_lm(C):
    """The cases' finite bigram table, float32."""
    return NR.random_lm(C, seed=7)


@functools.lru_cache(maxsize=None)
def case_inputs_ext(shape):
    """(logits (B, T, C) float32, in_len, lists, refs) of one nbest_ref.CASES shape: the
    restatement's uncollapsed lists (`case_inputs`) with the references of `pick_refs_ext`."""
    logits, in_len, lists, _ = case_inputs(shape)
    return logits, in_len, lists, pick_refs_ext(lists, shape[2])


def prior_kwargs(shape, table):
    return dict(lm=random_lm(shape[2]), lm_weight=LM_WEIGHT, length_bonus=LENGTH_BONUS) if table else {}


@functools.lru_cache(maxsize=None)
def case_ref_ext(shape, with_ref=True, table=True):
    """The restatement of one GPU case, computed once and shared."""
    logits, in_len, lists, refs = case_inputs_ext(shape)
    return mwer(logits, in_len, lists, refs, POSTERIOR_SCALE, n_max=shape[4], with_ref=with_ref,
                **prior_kwargs(shape, table))


def pack_lists(lists, N, H, fill=0):
    """Host arrays (tokens (B, N, H) int32, out_len (B, N), count (B)) in the decoder's format;
    unused cells hold `fill`."""
    B = len(lists)
    tokens = np.full((B, N, H), fill, np.int32)
    out_len = np.full((B, N), fill, np.int32)
    count = np.zeros(B, np.int32)
    for b, entries in enumerate(lists):
        count[b] = len(entries)
        for n, h in enumerate(entries):
            out_len[b, n] = len(h)
            tokens[b, n, :len(h)] = h
    return tokens, out_len, count


def pack_refs(refs):
    """(ref (B, R) int32 padded with 0, ref_len (B)), R >= 1."""
    R = max(1, max(len(r) for r in refs))
    ref = np.zeros((len(refs), R), np.int32)
    for b, r in enumerate(refs):
        ref[b, :len(r)] = r
    return ref, np.array([len(r) for r in refs], np.int32)
