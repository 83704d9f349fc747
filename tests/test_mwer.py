"""CPU checks of the MWER loss: the float64 restatement (tests/mwer_ref.py) against exhaustive
enumeration and against its own closed form, the conditions the GPU cases' inputs must meet,
host-only API validation, and the header's entry points.  No GPU, no library."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import decode_ref as D
from tests import mwer_ref as M
from tests import nbest_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(4, 3), (2, 6)]


def _logits(T, C, seed=1):
    return np.random.default_rng(seed).normal(0.0, 2.0, (T, C))


@pytest.mark.parametrize("T,C", SMALL)
def test_likelihood_of_every_labelling_equals_the_exhaustive_sum(T, C):
    x = _logits(T, C)
    paths = D.exhaustive(x)
    lp = M.log_probs(torch.tensor(x))
    for lab, want in paths.items():
        got = M.loglik(lp, T, list(lab))
        assert got is not None and abs(np.exp(float(got)) - np.exp(want)) < 1e-9, (lab, float(got), want)
    # a labelling that does not fit has no path
    assert M.loglik(lp, T, [1] * (T + 1)) is None and M.loglik(lp, 1, [1, 1]) is None
    assert M.fits([1, 1], 3) and not M.fits([1, 1], 2) and M.fits([], 0) and not M.fits([1], 0)


@pytest.mark.parametrize("T,C", SMALL)
def test_loss_and_gradient_over_all_labellings_equal_a_direct_enumeration(T, C):
    """With the list = every labelling and posterior_scale = 1 the posterior is the path
    distribution itself: loss = sum over all C^T paths of p(path) (err(labelling) - mean err)."""
    x = _logits(T, C, seed=2)
    labs = sorted(D.exhaustive(x))
    ref = [1, 2]
    res = M.mwer(x[None], [T], [[list(l) for l in labs]], [ref])
    err = {l: sum(D.wer_single(ref, list(l))[:3]) for l in labs}
    ebar = np.mean([err[l] for l in labs])
    xt = torch.tensor(x, requires_grad=True)
    lp = M.log_probs(xt)
    paths = list(itertools.product(range(C), repeat=T))
    idx = torch.tensor(paths)
    logp = lp[torch.arange(T), idx].sum(1)
    d = torch.tensor([err[tuple(c for c in D.collapse(p) if c != 0)] - ebar for p in paths], dtype=torch.float64)
    p = torch.softmax(logp, 0)
    loss = (p * d).sum()
    (g,) = torch.autograd.grad(loss, xt)
    assert abs(res["loss"] - float(loss.detach())) < 1e-9
    assert np.abs(res["dlogits"][0] - g.numpy()).max() < 1e-9
    assert abs(res["posterior"].sum() - 1.0) < 1e-12 and np.abs(res["dlogits"]).max() > 1e-3


@pytest.mark.parametrize("shape", list(NR.CASES), ids=[f"C{s[2]}" for s in NR.CASES])
def test_closed_form_gradient_equals_autograd_and_the_gpu_inputs_are_informative(shape):
    logits, in_len, lists, refs = M.case_inputs(shape)
    res = M.case_ref(shape)
    got = M.analytic_grad(logits, in_len, lists, refs, M.POSTERIOR_SCALE)
    assert np.abs(got - res["dlogits"]).max() < 1e-9
    for b, entries in enumerate(lists):
        assert len(set(map(tuple, entries))) == len(entries)  # uncollapsed lists hold distinct labellings
        if in_len[b] >= 1:
            errs = res["errors"][b, :len(entries)]
            assert errs.min() != errs.max(), (shape, b, errs)
            assert np.abs(res["dlogits"][b]).max() >= 1e-3, (shape, b, np.abs(res["dlogits"][b]).max())
            assert not res["dlogits"][b, in_len[b]:].any()
        else:
            assert not res["dlogits"][b].any() and res["loglik"][b, 0] == 0.0
    assert np.isfinite(res["loss"])


def test_equal_error_counts_give_no_gradient_and_unfit_entries_no_posterior():
    x = _logits(5, 4, seed=3)[None]
    res = M.mwer(x, [3], [[[1], [2], [3]]], [[1, 2, 3]])
    assert set(res["errors"][0]) == {2} and not res["dlogits"].any() and res["loss"] == 0.0
    res = M.mwer(x, [3], [[[1], [2, 2], [1, 2, 1, 2]]], [[1]])
    assert res["loglik"][0, 2] == -np.inf and res["posterior"][0, 2] == 0.0 and res["posterior"][0, :2].sum() == 1.0
    assert np.abs(M.analytic_grad(x, [3], [[[1], [2, 2], [1, 2, 1, 2]]], [[1]]) - res["dlogits"]).max() < 1e-12


def test_mwer_spec_validation():
    from scattennet_amd import MWER
    m = MWER(0.5, beam_size=8, nbest=3)
    assert (m.weight, m.beam_size, m.nbest, m.posterior_scale, m.head) == (0.5, 8, 3, 1.0, "fuse_coord_gloss_logits")
    assert MWER(1, beam_size=4).nbest == 4 and "nbest=3" in repr(m)
    for kw, match in ((dict(weight=-1.0), "weight"), (dict(weight=float("nan")), "weight"),
                      (dict(weight="x"), "numbers"), (dict(weight=1.0, beam_size=0), "beam_size"),
                      (dict(weight=1.0, beam_size=33), "beam_size"), (dict(weight=1.0, beam_size=True), "beam_size"),
                      (dict(weight=1.0, beam_size=4, nbest=5), "exceeds"), (dict(weight=1.0, nbest=0), "nbest"),
                      (dict(weight=1.0, posterior_scale=float("inf")), "posterior_scale"),
                      (dict(weight=1.0, head="logits"), "head")):
        with pytest.raises(ValueError, match=match):
            MWER(**kw)


def test_mwer_loss_host_validation():
    import scattennet_amd as S
    x = torch.zeros(2, 6, 5)
    il, lab, ll = torch.tensor([6, 4]), torch.tensor([[1, 2], [3, 0]]), torch.tensor([2, 1])
    with pytest.raises(RuntimeError, match="B, T, C"):
        S.mwer_loss(x[0], il, lab, ll)
    with pytest.raises(RuntimeError, match="input_lengths"):
        S.mwer_loss(x, torch.tensor([6, 7]), lab, ll)
    with pytest.raises(RuntimeError, match=r"\(B, R\)"):
        S.mwer_loss(x, il, lab[:1], ll)
    with pytest.raises(RuntimeError, match="gloss_lengths"):
        S.mwer_loss(x, il, lab, torch.tensor([2, 3]))
    with pytest.raises(RuntimeError, match="target values"):
        S.mwer_loss(x, il, torch.tensor([[1, 5], [3, 0]]), ll)
    with pytest.raises(ValueError, match="posterior_scale"):
        S.mwer_loss(x, il, lab, ll, posterior_scale=float("nan"))
    with pytest.raises(ValueError, match="beam_size"):
        S.mwer_loss(x, il, lab, ll, beam_size=40)
    with pytest.raises(ValueError, match="exceed the WER kernel's 128"):
        S.mwer_loss(torch.zeros(2, 130, 5), il, lab, ll)
    with pytest.raises(ValueError, match="WER kernel"):
        S.mwer_loss(x, il, torch.zeros(2, 129, dtype=torch.int64), ll)
    nb = S.NBest(torch.zeros(3, 4, 6, dtype=torch.int32), torch.zeros(3, 4, dtype=torch.int32), torch.zeros(3, 4),
                 torch.ones(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="single head"):
        S.mwer_loss(x, il, lab, ll, nbest=nb)
    with pytest.raises(RuntimeError, match="no CPU fallback|only on ROCm"):  # valid arguments, host tensors
        S.mwer_loss(x, il, lab, ll)
    for bad in ("x", 3):
        with pytest.raises(ValueError, match="MWER or None"):
            S.train_step(None, None, {}, mwer=bad)


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "scatten.h")).read()
    for name in ("sca_mwer_workspace_floats", "sca_mwer_fwd", "sca_mwer_bwd"):
        assert re.search(rf"\b(long|int) {name}\(", text), name
    from scattennet_amd import _lib
    assert {"sca_mwer_workspace_floats", "sca_mwer_fwd", "sca_mwer_bwd"} <= set(_lib.EXPORTS)
