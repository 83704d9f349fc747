"""N-best CTC decoding, bigram rescoring and MBR selection, host side (scattennet_amd/nbest.py;
sca_ctc_beam_decode_nbest, sca_nbest_rescore, sca_nbest_mbr, sca_nbest_gather of
include/scatten.h): the float64 restatements of tests/nbest_ref.py against the exhaustive
enumeration and hand cases, the tie margins of every GPU case's inputs, every argument error
before any device call, and the entry points' declarations.  CPU only.

Exact equality of a discrete search, a sort and an arg-min only means something away from ties,
so the inputs of tests/test_gpu_nbest.py are asserted here to keep MIN_GAP log units (risks:
MIN_GAP errors) in every per-frame cut, between neighbours of the final, merged and rescored
lists and between the two smallest risks.  That is a condition on the inputs (the seeds of
nbest_ref.CASES were chosen for it), not a tolerance."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import decode_ref as D
from tests import nbest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_GAP = 1e-4  # tests/test_decode.py
ENTRY_POINTS = {"sca_ctc_beam_decode_nbest": 14, "sca_ctc_beam_decode_heads_nbest": 15, "sca_nbest_rescore": 17,
                "sca_nbest_mbr": 12, "sca_nbest_gather": 13}
ERR_ARG = 1


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T,C", [(4, 3), (2, 6)])
def test_uncollapsed_list_equals_the_exhaustive_enumeration(T, C):
    """Every prefix fits a beam of 32, so the list is every labelling with its probability."""
    for seed in range(20):
        x = np.random.default_rng(100 + seed).normal(0.0, 2.0, (T, C))
        acc = D.exhaustive(x)
        want = sorted(acc.items(), key=lambda kv: -kv[1])
        entries, gaps = R.nbest(x, T, 32, 32, collapse_repeats=False)
        assert len(entries) == len(want) == (15 if (T, C) == (4, 3) else len(want)), seed
        assert gaps["final"] > 1e-9, seed  # no tie: the order is decided
        for (h, s), (lab, p) in zip(entries, want):
            assert tuple(h) == lab and abs(s - p) < 1e-9, (seed, h, lab)


@pytest.mark.parametrize("T,C,W", [(16, 4, 8), (20, 33, 32)])
def test_preselection_gives_the_same_list(T, C, W):
    x = np.random.default_rng(3).normal(0.0, 4.0, (T, C))
    a, _ = R.beam_search_all(x, T, W)
    b, _ = R.beam_search_all(x, T, W, preselect=True)
    assert [p for p, _ in a] == [p for p, _ in b] and len(a) == W
    assert max(abs(s - t) for (_, s), (_, t) in zip(a, b)) < 1e-9


def test_first_beam_is_the_one_best_restatement():
    x = np.random.default_rng(5).normal(0.0, 4.0, (12, 6))
    for collapse in (False, True):
        labels, score, _, _ = D.beam_search(x, 12, 8, collapse)
        beams, _ = R.beam_search_all(x, 12, 8)
        assert (D.collapse(list(beams[0][0])) if collapse else list(beams[0][0])) == labels
        assert abs(beams[0][1] - score) < 1e-12


def test_merging_hand_case():
    """(3) and (3, 3) collapse into one entry whose score is the logaddexp, and the order changes."""
    la = np.logaddexp
    entries = [((5,), math.log(0.40)), ((3,), math.log(0.35)), ((3, 3), math.log(0.20)), ((), math.log(0.05))]
    kept = R.merge_sort(entries, False)
    assert [h for h, _ in kept] == [[5], [3], [3, 3], []]
    merged = R.merge_sort(entries, True)
    assert [h for h, _ in merged] == [[3], [5], []]
    assert abs(merged[0][1] - la(math.log(0.35), math.log(0.20))) < 1e-15 and abs(merged[0][1] - math.log(0.55)) < 1e-12
    assert merged[1][1] == math.log(0.40) and merged[2][1] == math.log(0.05)
    # three into one, in entry order; equal scores keep their entry order (stable)
    three = R.merge_sort([((1, 1), -1.0), ((2,), -1.5), ((1,), -2.0), ((1, 1, 1), -3.0), ((4,), -1.5)], True)
    assert [h for h, _ in three] == [[1], [2], [4]]
    assert abs(three[0][1] - la(la(-1.0, -2.0), -3.0)) < 1e-15


def test_bigram_score_hand_cases():
    lm = np.arange(16, dtype=np.float64).reshape(4, 4) / 10.0  # lm[p, c] = (4 p + c) / 10
    assert R.bigram_score(lm, []) == lm[0, 0] == 0.0
    assert R.bigram_score(lm, [2]) == lm[0, 2] + lm[2, 0]
    assert abs(R.bigram_score(lm, [1, 3, 3]) - (lm[0, 1] + lm[1, 3] + lm[3, 3] + lm[3, 0])) < 1e-15
    entries = [([1, 3], -2.0), ([], -2.5), ([2], -3.0)]
    total, post, order = R.rescore(entries, lm, lm_weight=2.0, length_bonus=0.5, posterior_scale=1.0)
    want = [-2.0 + 2.0 * (0.1 + 0.7 + 1.2) + 1.0, -2.5 + 0.0, -3.0 + 2.0 * (0.2 + 0.8) + 0.5]
    assert np.allclose(total, want, rtol=0, atol=1e-15) and order == [0, 2, 1]
    assert abs(post.sum() - 1.0) < 1e-15 and np.allclose(post, np.exp(want) / np.exp(want).sum(), rtol=0, atol=1e-15)
    # no table: the identity, and the posterior of the scores; the scale flattens it
    total, post, order = R.rescore(entries)
    assert total.tolist() == [-2.0, -2.5, -3.0] and order == [0, 1, 2]
    flat = R.rescore(entries, posterior_scale=0.0)[1]
    assert np.allclose(flat, 1.0 / 3.0)


def test_mbr_hand_case():
    """The best-scoring hypothesis is an outlier; two close ones share the rest of the mass."""
    entries = [([1, 2, 3], 0.0), ([4, 5], 0.0), ([4, 6], 0.0)]
    post = np.array([0.4, 0.35, 0.25])
    loss, risk, best = R.mbr(entries, post)
    assert loss.tolist() == [[0, 3, 3], [3, 0, 1], [3, 1, 0]]  # (4, 5) -> (1, 2, 3): 2 sub + 1 del (or ins)
    assert np.allclose(risk, [0.6 * 3, 0.4 * 3 + 0.25, 0.4 * 3 + 0.35]) and best == 1
    # ties go to the lower entry
    assert R.mbr([([1], 0.0), ([2], 0.0)], np.array([0.5, 0.5]))[2] == 0
    # the loss is the project's alignment, not symmetric in general: ref (1) hyp () is a deletion
    assert R.mbr([([], 0.0), ([1], 0.0)], np.array([0.5, 0.5]))[0].tolist() == [[0, 1], [1, 0]]


def test_from_sequences_rows_normalise_and_match_hand_counts():
    import scattennet_amd as S
    seqs = [[1, 2], [1, 2, 2], [], [3]]
    n = S.BigramLM.counts(seqs, 4)
    assert n.tolist() == [[1, 2, 0, 1], [0, 0, 2, 0], [2, 0, 1, 0], [1, 0, 0, 0]]
    lm = S.BigramLM.from_sequences(seqs, 4, add_k=0.5)
    t = lm.table.double().numpy()
    assert lm.num_classes == 4 and lm.table.dtype == torch.float32 and lm.table.device.type == "cpu"
    assert np.abs(np.log(np.exp(t).sum(1))).max() < 1e-6
    assert abs(t[0, 1] - math.log(2.5 / 6.0)) < 1e-6 and abs(t[1, 2] - math.log(2.5 / 4.0)) < 1e-6
    assert abs(t[3, 3] - math.log(0.5 / 3.0)) < 1e-6
    big = S.BigramLM.from_sequences([[5, 7, 7]], 1124).table.double().numpy()
    assert np.abs(np.log(np.exp(big).sum(1))).max() < 1e-5
    for bad in ([[0]], [[4]], [[-1]]):
        with pytest.raises(ValueError, match="tokens must lie"):
            S.BigramLM.from_sequences(bad, 4)
    with pytest.raises(ValueError, match="add_k"):
        S.BigramLM.from_sequences(seqs, 4, add_k=0.0)
    with pytest.raises(ValueError, match=r"\(C, C\)"):
        S.BigramLM(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="finite"):
        S.BigramLM(np.full((3, 3), -np.inf, np.float32))


# -------------------------------------------------------------------- the GPU cases' inputs
@pytest.mark.parametrize("shape", list(R.CASES), ids=["B%d_T%d_C%d_W%d_N%d" % s for s in R.CASES])
def test_gpu_cases_are_away_from_ties(shape):
    lens = R.CASES[shape][1]
    assert len(lens) == shape[0] and max(lens) == shape[1]
    for collapse, rescored in ((True, True), (False, False)):
        ref = R.case_ref(shape, collapse, rescored)
        for b, clip in enumerate(ref):
            print(shape, collapse, b, len(clip["entries"]), {k: "%.2e" % v for k, v in clip["gaps"].items()})
            for name, gap in clip["gaps"].items():
                assert gap >= MIN_GAP, (shape, collapse, b, name, gap)
            assert 1 <= len(clip["entries"]) <= shape[4]
    counts = [len(c["entries"]) for c in R.case_ref(shape)]
    if 0 in lens:
        assert counts[lens.index(0)] == 1 and R.case_ref(shape)[lens.index(0)]["entries"][0] == ([], 0.0)


def test_gpu_cases_cover_merging_and_short_lists():
    merged = [len(c["entries"]) for c in R.case_ref((5, 16, 4, 8, 8))]
    plain = [len(c["entries"]) for c in R.case_ref((5, 16, 4, 8, 8), False, False)]
    assert sum(merged) < sum(plain) and max(plain) == 8 and min(merged) == 1  # merges; count < N
    assert any(c["order"] != sorted(c["order"]) for s in R.CASES for c in R.case_ref(s))  # rescoring reorders


def test_fixture_model_logits_are_away_from_ties():
    """The step tests of tests/test_gpu_nbest.py decode the fixture model's own logits; the
    fixture's recorded logits (the device's differ by rounding) keep the margins at MODEL_BEAM,
    and MBR picks another entry than the best total somewhere."""
    from tests.golden_util import load
    fx = load("model_small", "manifest_model.json")
    lens = fx["out.input_lengths"].numpy()
    differs = False
    for key in ("alignment_gloss_logits", "fuse_coord_gloss_logits"):
        res = R.full(fx["out." + key].double().numpy(), lens, R.MODEL_BEAM, 3, True, R.random_lm(fx["meta"]["vocab"]),
                     R.LM_WEIGHT, R.LENGTH_BONUS, R.POSTERIOR_SCALE)
        for clip in res:
            assert min(clip["gaps"].values()) >= MIN_GAP, (key, clip["gaps"])
            differs |= clip["best"] != clip["order"][0]
    assert differs


# ------------------------------------------------------------------------- the entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    from scattennet_amd import _lib
    src = _header()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, nargs in ENTRY_POINTS.items():
        assert re.search(r"^\s*int\s+%s\s*\(" % name, src, flags=re.M), name
        assert name in _lib.EXPORTS, name
        declared = len(re.search(r"%s\s*\((.*?)\)" % name, src, flags=re.S).group(1).split(","))
        assert len(_lib.EXPORTS[name][0]) == declared == nargs, name
        assert hasattr(lib, name), name
        assert name in doc, name


def _bound():
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ENTRY_POINTS:
        getattr(lib, name).argtypes, getattr(lib, name).restype = L.EXPORTS[name]
    return L, lib


def test_c_argument_validation_makes_no_gpu_call():
    L, lib = _bound()
    p = ctypes.c_void_p(0x1000)

    def one(B=2, T=8, C=16, W=5, N=3, logits=p, count=p):
        return lib.sca_ctc_beam_decode_nbest(logits, p, B, T, C, W, N, 1, p, p, p, count, p, None)
    assert one(N=0) == ERR_ARG and one(N=6) == ERR_ARG and one(W=33, N=33) == ERR_ARG and one(W=0, N=0) == ERR_ARG
    assert one(C=8193) == ERR_ARG and one(B=0) == ERR_ARG and one(T=0) == ERR_ARG
    assert one(logits=None) == ERR_ARG and one(count=None) == ERR_ARG
    hx = L.DecodeHeads()
    for g in range(8):
        hx.logits[g] = 0x1000

    def heads(G=2, W=5, N=3, h=hx):
        return lib.sca_ctc_beam_decode_heads_nbest(ctypes.byref(h), G, p, 2, 8, 16, W, N, 1, p, p, p, p, p, None)
    assert heads(G=0) == ERR_ARG and heads(G=9) == ERR_ARG and heads(N=6) == ERR_ARG and heads(N=0) == ERR_ARG
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000
    assert heads(h=hole) == ERR_ARG

    def rescore(G=2, B=2, N=3, T=8, lm=p, C=16, lw=0.5, lb=0.0, ps=1.0, total=p):
        return lib.sca_nbest_rescore(p, p, p, p, G, B, N, T, lm, C, lw, lb, ps, total, p, p, None)
    assert rescore(N=0) == ERR_ARG and rescore(N=33) == ERR_ARG and rescore(G=9) == ERR_ARG and rescore(B=0) == ERR_ARG
    assert rescore(T=0) == ERR_ARG and rescore(C=0) == ERR_ARG and rescore(C=8193) == ERR_ARG
    assert rescore(total=None) == ERR_ARG
    for bad in (float("nan"), float("inf")):
        assert rescore(lw=bad) == ERR_ARG and rescore(lb=bad) == ERR_ARG and rescore(ps=bad) == ERR_ARG

    def mbr(G=2, B=2, N=3, T=8, loss=p):
        return lib.sca_nbest_mbr(p, p, p, p, G, B, N, T, loss, p, p, None)
    assert mbr(T=129) == ERR_ARG and mbr(N=33) == ERR_ARG and mbr(N=0) == ERR_ARG and mbr(loss=None) == ERR_ARG

    def gather(stride=1, N=3, sel=p):
        return lib.sca_nbest_gather(p, p, p, sel, stride, 2, 2, N, 8, p, p, p, None)
    assert gather(stride=0) == ERR_ARG and gather(stride=4) == ERR_ARG and gather(N=33) == ERR_ARG
    assert gather(sel=None) == ERR_ARG
    with pytest.raises(ValueError, match="sca_nbest_mbr"):
        L.check(mbr(T=129), "sca_nbest_mbr")


# ------------------------------------------------------------------------ Python validation
def test_python_validation_comes_before_the_device():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    il = torch.tensor([8, 5])
    for fn, arg in ((S.ctc_decode_nbest_device, x), (S.ctc_decode_nbest_heads_device, [x, x])):
        with pytest.raises(ValueError, match="beam_size must lie"):
            fn(arg, il, 0)
        with pytest.raises(ValueError, match="beam_size must lie"):
            fn(arg, il, 33)
        with pytest.raises(ValueError, match="nbest must lie"):
            fn(arg, il, 5, nbest=6)
        with pytest.raises(ValueError, match="nbest must lie"):
            fn(arg, il, 5, nbest=0)
        with pytest.raises(RuntimeError, match="at most 8"):
            fn(arg, torch.tensor([9, 5]), 5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(arg, il, 5, nbest=3)
    with pytest.raises(ValueError, match="same shape"):
        S.ctc_decode_nbest_heads_device([x, torch.randn(2, 8, 13)], il, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_decode_nbest(x, 5, il)
    nb = S.NBest(torch.zeros(2, 3, 8, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3),
                 torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="lm must be a BigramLM"):
        S.rescore_nbest_device(nb, lm=np.zeros((12, 12)))
    with pytest.raises(ValueError, match="lm_weight must be finite"):
        S.rescore_nbest_device(nb, lm_weight=float("nan"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.rescore_nbest_device(nb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.mbr_select_device(nb, torch.zeros(2, 3))
    wide = S.NBest(torch.zeros(2, 3, 129, dtype=torch.int32), nb.lengths, nb.scores, nb.count)
    with pytest.raises(ValueError, match="exceed the WER kernel's 128"):
        S.mbr_select_device(wide, torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="do not fit"):
        S.rescore_nbest_device(S.NBest(nb.tokens, nb.lengths, torch.zeros(2, 4), nb.count))


def test_rescoring_spec_validation():
    import scattennet_amd as S
    lm = S.BigramLM(R.random_lm(12))
    spec = S.Rescoring(3, lm, 0.5, 0.1, select="mbr")
    assert (spec.nbest, spec.lm_weight, spec.length_bonus, spec.posterior_scale, spec.select) == (3, 0.5, 0.1, 1.0, "mbr")
    assert "nbest=3" in repr(spec)
    for bad in (0, 33, 2.0, True, None):
        with pytest.raises(ValueError, match="nbest must be an int"):
            S.Rescoring(bad)
    with pytest.raises(ValueError, match="select must be one of"):
        S.Rescoring(3, select="risk")
    with pytest.raises(ValueError, match="lm must be a BigramLM"):
        S.Rescoring(3, lm=torch.zeros(4, 4))
    with pytest.raises(ValueError, match="posterior_scale must be finite"):
        S.Rescoring(3, posterior_scale=float("inf"))
    x = torch.randn(2, 8, 12)
    il = torch.tensor([8, 5])
    with pytest.raises(ValueError, match="nbest = 3 exceeds beam_size = 2"):
        S.rescored_decode([x], il, 2, spec)
    with pytest.raises(ValueError, match="needs a beam search"):
        S.rescored_decode([x], il, 0, spec)
    with pytest.raises(ValueError, match="12 classes, the logits 13"):
        S.rescored_decode([torch.randn(2, 8, 13)], il, 5, spec)
    with pytest.raises(ValueError, match="129 logit frames exceeds"):
        S.rescored_decode([torch.randn(2, 129, 12)], torch.tensor([129, 5]), 5, spec)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.rescored_decode([x], il, 5, spec)
    # the steps validate the spec on the host too
    outputs = {"alignment_gloss_logits": x, "input_lengths": il}
    with pytest.raises(ValueError, match="nbest = 3 exceeds beam_size = 1"):
        S.decode_outputs(outputs, 1, rescoring=spec)
    with pytest.raises(ValueError, match="rescoring must be a Rescoring"):
        S.eval_step(None, None, None, rescoring={"nbest": 3})
    with pytest.raises(ValueError, match="recognize_step: rescoring.nbest = 3 exceeds beam_size = 2"):
        S.recognize_step(None, None, beam_size=2, rescoring=spec)


def test_nbest_lists_orders_and_cuts():
    from scattennet_amd.nbest import nbest_lists
    tokens = np.array([[[1, 2, 0], [3, 0, 0], [0, 0, 0]]])
    lists = nbest_lists(tokens, np.array([[2, 1, 0]]), np.array([[-1.0, -0.5, -np.inf]]), np.array([2]),
                        np.array([[0.4, 0.6, 0.0]]), np.array([[1, 0, 2]]))
    assert lists == [[([3], -0.5, 0.6), ([1, 2], -1.0, 0.4)]]
    assert nbest_lists(tokens, np.array([[2, 1, 0]]), np.array([[-1.0, -0.5, 0.0]]), np.array([3])) == \
        [[([1, 2], -1.0), ([3], -0.5), ([], 0.0)]]
