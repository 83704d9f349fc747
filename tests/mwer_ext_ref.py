"""float64 restatement for tests/test_mwer_ext.py and tests/test_gpu_mwer_ext.py of the extended
MWER loss as include/scatten.h specifies it (sca_mwer_heads_fwd / sca_mwer_heads_bwd): the
n-best list with the clip's reference as one more slot, the bigram gloss model and the length
bonus inside the posterior.  Built on tests/mwer_ref.py (`loglik`, `fits`, `alpha_beta`) and
decode_ref.wer_single; the gradient by torch.autograd, and `analytic_grad` restates the header's
closed form over the enlarged list so that the two can be compared.  A grouped call is this
restatement once per head.  Also the inputs the GPU cases share.  No part of the package is
used."""
import functools

import numpy as np
import torch

from tests import decode_ref as D
from tests import mwer_ref as M
from tests import nbest_ref as NR

NEG_INF = -np.inf
LM_WEIGHT, LENGTH_BONUS = 0.7, 0.3  # the cases'


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
    ok = M.fits([int(v) for v in ref], Tb) and 0 not in errs
    return labels + [[int(v) for v in ref]], errs + [0], ok


def mwer(logits, in_lens, lists, refs, posterior_scale=1.0, n_max=None, with_ref=False, lm=None, lm_weight=0.0,
         length_bonus=0.0, grad=True):
    """One head's loss: mwer_ref.mwer with M = n_max + with_ref slots per clip.  loglik, posterior
    and errors are (B, M); loglik[b, N] is the reference's whenever it fits, also where the slot
    is a duplicate; ref_valid (B) int64; risk (B), loss, and with `grad` dlogits (B, T, C)."""
    x = torch.tensor(np.asarray(logits), dtype=torch.float64, requires_grad=True)
    B, T, _ = x.shape
    N = n_max or max(len(l) for l in lists)
    Ms = N + (1 if with_ref else 0)
    lp = M.log_probs(x)
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
            ll = M.loglik(lp[b], Tb, h)
            if ll is None:
                continue
            out["loglik"][b, n] = float(ll.detach())
            if is_ref and not ref_ok:
                continue
            valid.append(n)
            zs.append(ll + prior(h, lm, lm_weight, length_bonus))
        if not valid:
            continue
        post, risk, loss_b = M.clip_stats(torch.stack(zs), [out["errors"][b, n] for n in valid], posterior_scale)
        out["posterior"][b, valid] = post.detach().numpy()
        out["risk"][b] = float(risk.detach())
        loss = loss + loss_b / B
    out["loss"] = float(loss.detach())
    if grad:
        out["dlogits"] = torch.autograd.grad(loss, x)[0].numpy() if loss.requires_grad else np.zeros(x.shape)
    return out


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
        keep = [k for k, h in enumerate(labels) if M.fits(h, Tb)]
        if len(keep) < 2 or Tb == 0:
            continue
        ent = [labels[k] for k in keep]
        err = np.array([errs[k] for k in keep], np.float64)
        ab = [M.alpha_beta(lp[b], Tb, h) for h in ent]
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
def pick_refs(lists, C):
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
def case_inputs(shape):
    """(logits (B, T, C) float32, in_len, lists, refs) of one nbest_ref.CASES shape: the
    restatement's uncollapsed lists (mwer_ref.case_inputs) with the references of `pick_refs`."""
    logits, in_len, lists, _ = M.case_inputs(shape)
    return logits, in_len, lists, pick_refs(lists, shape[2])


def prior_kwargs(shape, table):
    return dict(lm=random_lm(shape[2]), lm_weight=LM_WEIGHT, length_bonus=LENGTH_BONUS) if table else {}


@functools.lru_cache(maxsize=None)
def case_ref(shape, with_ref=True, table=True):
    """The restatement of one GPU case, computed once and shared."""
    logits, in_len, lists, refs = case_inputs(shape)
    return mwer(logits, in_len, lists, refs, M.POSTERIOR_SCALE, n_max=shape[4], with_ref=with_ref,
                **prior_kwargs(shape, table))
