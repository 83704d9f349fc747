"""CPU checks of the extended MWER loss (the reference as one more entry of the list, the gloss
model's prior inside the posterior, several heads per call): the float64 restatement
(tests/mwer_ref.py) against its own closed form, the slot rules, the conditions the GPU
cases' inputs must meet, host-only API validation, and the header's entry points.  No GPU."""
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
SHAPES = list(NR.CASES)
IDS = [f"C{s[2]}" for s in SHAPES]


def _logits(T, C, seed=1):
    return np.random.default_rng(seed).normal(0.0, 2.0, (T, C))


@pytest.mark.parametrize("table", [False, True], ids=["acoustic", "table"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_closed_form_gradient_equals_autograd_on_the_augmented_lists(shape, table):
    logits, in_len, lists, refs = M.case_inputs_ext(shape)
    res = M.case_ref_ext(shape, True, table)
    got = M.analytic_grad(logits, in_len, lists, refs, M.POSTERIOR_SCALE, with_ref=True, **M.prior_kwargs(shape, table))
    assert np.abs(got - res["dlogits"]).max() < 1e-9
    assert np.isfinite(res["loss"]) and np.abs(res["dlogits"]).max() >= 1e-3


def test_the_gpu_inputs_cover_the_slot_rules():
    """One valid reference slot per case; a duplicate, an unfit reference, a 33-slot clip and a
    reference as long as its clip somewhere across the cases; the slot changes every loss."""
    seen = {"duplicate": 0, "unfit": 0, "slots33": 0, "full_length": 0}
    for shape in SHAPES:
        B, T, C, W, N = shape
        logits, in_len, lists, refs = M.case_inputs_ext(shape)
        res = M.case_ref_ext(shape, True, False)
        assert res["ref_valid"].sum() >= 1, shape
        assert abs(res["loss"] - M.case_ref_ext(shape, False, False)["loss"]) > 1e-6, shape
        for b in range(B):
            assert all(1 <= c < C for c in refs[b])
            fits = M.fits(refs[b], in_len[b])
            dup = refs[b] in lists[b]
            assert res["ref_valid"][b] == int(fits and not dup), (shape, b)
            assert np.isfinite(res["loglik"][b, N]) == fits and res["errors"][b, N] == 0
            seen["duplicate"] += fits and dup
            seen["unfit"] += not fits
            seen["slots33"] += bool(res["ref_valid"][b]) and len(lists[b]) == 32
            seen["full_length"] += fits and len(refs[b]) == in_len[b]
            if res["ref_valid"][b]:
                assert res["posterior"][b, N] > 0 and np.abs(res["dlogits"][b]).max() > 0
            else:
                assert res["posterior"][b, N] == 0
    print(seen)
    assert all(v >= 1 for v in seen.values()), seen


def test_error_count_zero_means_equal_sequences():
    """The duplicate rule rests on it: under wer_single's costs err == 0 iff the sequences are equal."""
    pairs = 0
    for shape in SHAPES:
        _, _, lists, refs = M.case_inputs_ext(shape)
        pool = [list(r) for r in refs] + [list(r) for r in M.case_inputs(shape)[3]]
        for b, entries in enumerate(lists):
            for r in pool:
                for h in entries:
                    assert (sum(D.wer_single(list(r), list(h))[:3]) == 0) == (list(r) == list(h)), (r, h)
                    pairs += 1
    seqs = [list(s) for n in range(4) for s in itertools.product((1, 2), repeat=n)]
    for r, h in itertools.product(seqs, seqs):
        assert (sum(D.wer_single(r, h)[:3]) == 0) == (r == h), (r, h)
    assert pairs > 500


def test_slot_rules():
    x = _logits(5, 4, seed=3)[None]
    kw = dict(with_ref=True)
    # a duplicate: the slot is out of V, its likelihood is still reported, the result is the plain list's
    res, plain = M.mwer(x, [4], [[[1], [2, 3]]], [[2, 3]], **kw), M.mwer(x, [4], [[[1], [2, 3]]], [[2, 3]])
    assert res["ref_valid"][0] == 0 and res["posterior"][0, 2] == 0.0
    assert res["loglik"][0, 2] == res["loglik"][0, 1] and np.isfinite(res["loglik"][0, 2])
    assert res["loss"] == plain["loss"] and np.array_equal(res["dlogits"], plain["dlogits"])
    # an unfit reference ([1, 1] needs 3 frames)
    res = M.mwer(x, [2], [[[1], [2]]], [[1, 1]], **kw)
    assert res["ref_valid"][0] == 0 and res["loglik"][0, 2] == -np.inf and res["posterior"][0, 2] == 0.0
    # an empty reference: valid iff the empty entry is absent
    assert M.mwer(x, [3], [[[1], [2]]], [[]], **kw)["ref_valid"][0] == 1
    assert M.mwer(x, [3], [[[1], []]], [[]], **kw)["ref_valid"][0] == 0
    assert M.mwer(x, [0], [[[]]], [[]], **kw)["ref_valid"][0] == 0 and M.mwer(x, [0], [[[1]]], [[]], **kw)["ref_valid"][0] == 1
    # count = 0 with a fitting reference: a lone valid slot, posterior 1, no loss and no gradient
    res = M.mwer(x, [5], [[]], [[1, 2]], n_max=2, **kw)
    assert res["ref_valid"][0] == 1 and res["posterior"][0].tolist() == [0.0, 0.0, 1.0]
    assert res["loss"] == 0.0 and res["risk"][0] == 0.0 and not res["dlogits"].any()
    assert not M.analytic_grad(x, [5], [[]], [[1, 2]], **kw).any()
    # equal error counts have no gradient without the slot and one with it
    lists, refs = [[[1], [2], [3]]], [[1, 2, 3]]
    assert not M.mwer(x, [5], lists, refs)["dlogits"].any()
    res = M.mwer(x, [5], lists, refs, **kw)
    assert set(res["errors"][0, :3]) == {2} and np.abs(res["dlogits"]).max() > 1e-3 and res["loss"] != 0
    assert np.abs(M.analytic_grad(x, [5], lists, refs, **kw) - res["dlogits"]).max() < 1e-12


def test_prior_is_the_rescorers_total_and_weight_zero_changes_nothing():
    x = _logits(6, 5, seed=4)[None]
    lists, refs = [[[1, 2], [3], [], [4, 4]]], [[1, 3]]
    lm = NR.random_lm(5, seed=2)
    base = M.mwer(x, [6], lists, refs, 0.8, with_ref=True)
    zero = M.mwer(x, [6], lists, refs, 0.8, with_ref=True, lm=lm, lm_weight=0.0, length_bonus=0.0)
    assert zero["loss"] == base["loss"] and np.array_equal(zero["posterior"], base["posterior"])
    res = M.mwer(x, [6], lists, refs, 0.8, with_ref=True, lm=lm, lm_weight=0.7, length_bonus=0.3)
    slots = lists[0] + refs
    total, post, _ = NR.rescore([(h, ll) for h, ll in zip(slots, res["loglik"][0])], lm, 0.7, 0.3, 0.8)
    assert np.abs(post - res["posterior"][0]).max() < 1e-12 and abs(res["loss"] - base["loss"]) > 1e-4
    assert M.prior([], lm, 0.7, 0.3) == pytest.approx(0.7 * lm[0, 0])


def test_mwer_spec_validation_and_repr():
    from scattennet_amd import MWER, BigramLM
    both = ("alignment_gloss_logits", "fuse_coord_gloss_logits")
    assert repr(MWER(0.5, beam_size=8, nbest=3)) == ("MWER(weight=0.5, beam_size=8, nbest=3, posterior_scale=1.0, "
                                                      "head='fuse_coord_gloss_logits')")
    lm = BigramLM(torch.zeros(4, 4))
    m = MWER(0.5, beam_size=8, nbest=3, reference=True, head=both, lm=lm, lm_weight=0.5)
    assert m.heads == both and m.head == both and m.reference and m.lm is lm and m.lm_weight == 0.5 and not m.fusion
    assert "reference=True" in repr(m) and "lm_weight=0.5" in repr(m) and "length_bonus" not in repr(m)
    assert MWER(1.0).heads == ("fuse_coord_gloss_logits",) and MWER(1.0).head == "fuse_coord_gloss_logits"
    assert MWER(1.0, lm=np.zeros((3, 3), np.float32)).lm.num_classes == 3
    for kw, match in ((dict(head=both + both[:1]), "distinct"), (dict(head=("logits",)), "head"),
                      (dict(head=()), "between 1 and 8"), (dict(head=both * 5), "between 1 and 8"),
                      (dict(head=(3,)), "head"), (dict(lm=torch.zeros(3, 4)), r"\(C, C\)"),
                      (dict(lm=torch.full((3, 3), float("nan"))), "finite"), (dict(lm="table"), "lm must be"),
                      (dict(lm_weight=float("nan")), "lm_weight"), (dict(length_bonus=float("inf")), "length_bonus"),
                      (dict(lm_weight=None), "numbers"), (dict(fusion=True), "nothing to fuse"),
                      (dict(fusion=1, lm=lm), "bool"), (dict(reference=1), "bool")):
        with pytest.raises(ValueError, match=match):
            MWER(1.0, **kw)


def test_mwer_loss_host_validation():
    import scattennet_amd as S
    x = torch.zeros(2, 6, 5)
    il, lab, ll = torch.tensor([6, 4]), torch.tensor([[1, 2], [3, 0]]), torch.tensor([2, 1])
    lm = S.BigramLM(torch.zeros(5, 5))
    with pytest.raises(ValueError, match=r"\(C, C\)"):
        S.mwer_loss(x, il, lab, ll, lm=torch.zeros(5, 4))
    with pytest.raises(ValueError, match="the gloss model has 4 classes, the logits 5"):
        S.mwer_loss(x, il, lab, ll, lm=S.BigramLM(torch.zeros(4, 4)))
    with pytest.raises(ValueError, match="lm_weight"):
        S.mwer_loss(x, il, lab, ll, lm=lm, lm_weight=float("inf"))
    with pytest.raises(ValueError, match="length_bonus"):
        S.mwer_loss(x, il, lab, ll, length_bonus=float("nan"))
    with pytest.raises(ValueError, match="nothing to fuse"):
        S.mwer_loss(x, il, lab, ll, fusion=True)
    with pytest.raises(ValueError, match="reference must be a bool"):
        S.mwer_loss(x, il, lab, ll, reference=1)
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.mwer_loss([x] * 9, il, lab, ll)
    with pytest.raises(ValueError, match="same shape"):
        S.mwer_loss([x, x[:, :5]], il, lab, ll)
    single = S.NBest(torch.zeros(2, 4, 6, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4),
                     torch.ones(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="the 2 heads'"):
        S.mwer_loss([x, x], il, lab, ll, nbest=single)
    with pytest.raises(ValueError, match="does not go with nbest"):
        S.mwer_loss(x, il, lab, ll, nbest=single, lm=lm, fusion=True)
    with pytest.raises(RuntimeError, match=r"\(B, R\)"):
        S.mwer_loss([x, x], il, lab[:1], ll, reference=True)
    for kw in (dict(reference=True), dict(lm=lm, lm_weight=0.5)):  # valid arguments, host tensors
        with pytest.raises(RuntimeError, match="no CPU fallback|only on ROCm"):
            S.mwer_loss(x, il, lab, ll, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback|only on ROCm"):
        S.mwer_loss([x, x], il, lab, ll)


def test_header_declares_and_the_library_exports_the_entry_points():
    import ctypes
    text = open(os.path.join(ROOT, "include", "scatten.h")).read()
    names = ("sca_mwer_heads_workspace_floats", "sca_mwer_heads_fwd", "sca_mwer_heads_bwd")
    for name in names:
        assert re.search(rf"\b(long|int) {name}\(", text), name
    assert "sca_mwer_grads" in text
    from scattennet_amd import _lib
    assert set(names) <= set(_lib.EXPORTS)
    assert ctypes.sizeof(_lib.MwerGrads) == 8 * _lib.EVAL_MAX_HEADS
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ws = lib.sca_mwer_heads_workspace_floats
    ws.restype, old = ctypes.c_long, lib.sca_mwer_workspace_floats
    old.restype = ctypes.c_long
    # the old layout is a prefix: G = 1 without the reference adds the prior's B N floats only
    assert ws(1, 8, 5, 64, 64, 24, 0) == old(8, 5, 64, 64) + 8 * 5
    assert ws(2, 8, 5, 64, 64, 80, 1) == 2 * (2 * 8 * 64 + 2 * 8 * 6 * 64 * 161 + 3 * 8 * 6 + 8)
    assert ws(0, 8, 5, 64, 64, 24, 0) == 0
    # arguments are validated before any GPU call: NULL pointers and bad sizes are SCA_ERR_ARG
    fwd, bwd = lib.sca_mwer_heads_fwd, lib.sca_mwer_heads_bwd
    fwd.argtypes, bwd.argtypes = _lib.EXPORTS["sca_mwer_heads_fwd"][0], _lib.EXPORTS["sca_mwer_heads_bwd"][0]
    hx = _lib.DecodeHeads()
    assert fwd(ctypes.byref(hx), 1, *[None] * 6, 2, 3, 4, 5, 4, 2, 1, None, 0.0, 0.0, 1.0, *[None] * 8) == 1
    assert fwd(ctypes.byref(hx), 9, *[None] * 6, 2, 3, 4, 5, 4, 2, 1, None, 0.0, 0.0, 1.0, *[None] * 8) == 1
    assert bwd(ctypes.byref(hx), 1, *[None] * 6, 2, 3, 4, 5, 4, 2, 1, *[None] * 4) == 1
