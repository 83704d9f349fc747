"""Shallow fusion of the bigram gloss model into the CTC beam search, host side
(sca_ctc_beam_decode_fused_nbest of include/scatten.h; scattennet_amd/nbest.py): the float64
restatement of tests/fusion_ref.py against the exhaustive enumeration, the unfused restatement
and the rescorer, the exactness of the per-beam preselection (and a case in which the frame-wide
list is wrong), a case in which fusion finds a better total than rescoring, the tie margins of
every GPU case's inputs, and the argument errors of `Rescoring(fusion=...)`.  CPU only.

Exact equality of a discrete search only means something away from ties, so the inputs of
tests/test_gpu_fusion.py are asserted here to keep MIN_GAP log units in every per-frame cut and
between neighbours of the final, merged and rescored lists, and to give the same lists in
float32.  That is a condition on the inputs (the seeds were chosen for it), not a tolerance."""
import numpy as np
import pytest

from tests import decode_ref as D
from tests import fusion_ref as F
from tests import nbest_ref as R

MIN_GAP = 1e-4  # tests/test_decode.py


def _labels(entries):
    return [list(h) for h, _ in entries]


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("T,C", [(4, 3), (2, 6)])
def test_uncollapsed_fused_list_equals_the_exhaustive_enumeration(T, C):
    """Every prefix fits a beam of 32, so the list is every labelling, ordered by
    log p(h) + lm_weight * lm(h) + length_bonus * len(h) with the opening and closing terms."""
    for seed in range(12):
        rng = np.random.default_rng(200 + seed)
        x = rng.normal(0.0, 2.0, (T, C))
        lm = rng.normal(-2.0, 1.5, (C, C))
        acc = D.exhaustive(x)
        for w, bonus in ((0.5, 0.2), (3.0, -0.4), (-1.5, 0.0), (0.0, 0.7)):
            key = {h: p + w * R.bigram_score(lm, h) + bonus * len(h) for h, p in acc.items()}
            want = sorted(acc, key=lambda h: -key[h])
            beams, _, final_gap = F.search(x, T, 32, lm, w, bonus)
            assert len(beams) == len(want), (seed, w)
            assert final_gap > 1e-9, (seed, w)  # no tie: the order is decided
            for (p, tot, k), h in zip(beams, want):
                assert p == h and abs(tot - acc[h]) < 1e-9 and abs(k - key[h]) < 1e-9, (seed, w, p, h)


@pytest.mark.parametrize("T,C,W", [(16, 4, 8), (12, 6, 8), (20, 33, 32)])
def test_weight_zero_is_the_unfused_restatement(T, C, W):
    x = np.random.default_rng(3).normal(0.0, 4.0, (T, C))
    lm = R.random_lm(C)
    for collapse in (False, True):
        want, _ = R.nbest(x, T, W, W, collapse)
        for table in (None, lm):
            for preselect in F.PRESELECT:
                got, keys, _ = F.fused_nbest(x, T, W, W, collapse, table, 0.0, 0.0, preselect)
                assert _labels(got) == _labels(want)
                assert [s for _, s in got] == [s for _, s in want]
    beams, _, _ = F.search(x, T, W, lm, 0.0, 0.0)
    assert [k for _, _, k in beams] == [t for _, t, _ in beams]


def test_final_keys_are_the_rescorers_totals():
    x = np.random.default_rng(8).normal(0.0, 3.0, (14, 7))
    lm = R.random_lm(7).astype(np.float64)  # bigram_score sums in the table's type
    for w, bonus in ((0.5, 0.2), (3.0, 0.0), (-0.7, 0.3)):
        entries, keys, _ = F.fused_nbest(x, 14, 6, 6, False, lm, w, bonus)
        total, _, order = R.rescore(entries, lm, w, bonus)
        assert np.abs(total - np.array(keys)).max() < 1e-9
        assert order == list(range(len(entries)))  # the list is already in the rescorer's order


def test_in_len_zero_and_one():
    x = np.random.default_rng(1).normal(0.0, 2.0, (5, 4))
    lm = R.random_lm(4)
    entries, keys, _ = F.fused_nbest(x, 0, 3, 3, True, lm, 0.5, 0.2)
    assert entries == [([], 0.0)] and abs(keys[0] - 0.5 * lm[0, 0]) < 1e-12
    entries, _, _ = F.fused_nbest(x, 1, 3, 3, True, lm, 0.5, 0.2)
    assert len(entries) == 3 and all(len(h) <= 1 for h, _ in entries)


# ---------------------------------------------------------------------------- preselection
@pytest.mark.parametrize("T,C,W", [(64, 1124, 5), (37, 70, 1), (20, 33, 32), (16, 4, 8)])
@pytest.mark.parametrize("w", [0.3, 3.0])
def test_per_beam_preselection_is_exact(T, C, W, w):
    x = np.random.default_rng(4).normal(0.0, 4.0, (T, C))
    lm = R.random_lm(C)
    a, _, _ = F.search(x, T, W, lm, w, F.BONUS, None)
    b, _, _ = F.search(x, T, W, lm, w, F.BONUS, "per_beam")
    assert [p for p, _, _ in a] == [p for p, _, _ in b] and len(a) == min(W, len(a))
    assert max(abs(s - t) for (_, s, _), (_, t, _) in zip(a, b)) < 1e-9
    assert max(abs(s - t) for (_, _, s), (_, _, t) in zip(a, b)) < 1e-9


def test_shared_preselection_is_wrong_in_the_constructed_case():
    """Label 9 is outside frame 1's top-(W + 1) by lp and enters the beam through lm[1, 9]."""
    x, lm, w, W = F.constructed_case()
    lp = D.log_softmax(x[0])
    top = (np.argsort(-lp[1, 1:], kind="stable") + 1)[:W + 1]
    assert 9 not in top
    exact, gap, _ = F.search(x[0], 3, W, lm, w, 0.0, None)
    per_beam, _, _ = F.search(x[0], 3, W, lm, w, 0.0, "per_beam")
    shared, _, _ = F.search(x[0], 3, W, lm, w, 0.0, "shared")
    assert gap > MIN_GAP
    assert [p for p, _, _ in exact] == [p for p, _, _ in per_beam]
    assert (1, 9) in [p for p, _, _ in exact]
    assert [p for p, _, _ in shared] != [p for p, _, _ in exact]  # the case bites


def test_fallback_case_overflows_the_kernels_list():
    x, lm, w, _ = F.fallback_case()
    _, T, C, W, _ = F.FALLBACK_SHAPE
    lp = D.log_softmax(x[0])
    assert F.labels_over_threshold(lp[0], lm[0], w, W + 1) > F.FALLBACK_LIST
    assert F.labels_over_threshold(D.log_softmax(F.case_logits((2, 64, 1124, 5, 5))[0])[0], lm[0], w, 6) < 64


# ---------------------------------------------------------------- the point of the feature
WINS_MARGIN = 1.0


def test_fusion_finds_a_better_total_than_rescoring():
    """At beam 3 the unfused search prunes what the gloss model prefers; a second pass cannot
    bring it back.  Measured margin of this seeded case: 66.7 log units."""
    x, lm, w, bonus, W = F.wins_case()
    T = x.shape[1]
    _, keys, gaps = F.fused_nbest(x[0], T, W, W, False, lm, w, bonus, "per_beam")
    unfused, ugaps = R.nbest(x[0], T, W, W, False)
    total, _, _ = R.rescore(unfused, lm, w, bonus)
    assert min(gaps["frame"], gaps["final"], ugaps["frame"], ugaps["final"]) > MIN_GAP
    assert max(keys) - total.max() > WINS_MARGIN, (max(keys), total.max())


# ------------------------------------------------------------------- the GPU cases' inputs
@pytest.mark.parametrize("shape", list(F.CASES))
@pytest.mark.parametrize("w", F.WEIGHTS)
def test_gpu_case_inputs_are_away_from_ties_and_stable_in_float32(shape, w):
    for collapse in (True, False):
        ref = F.case_ref(shape, w, collapse)
        ref32 = F.case_ref(shape, w, collapse, np.float32)
        names = ("frame", "final", "total", "risk") + (("merged",) if collapse else ())
        for b, (r, r32) in enumerate(zip(ref, ref32)):
            for name in names:
                assert r["gaps"][name] > MIN_GAP, (shape, w, collapse, b, name, r["gaps"][name])
            assert _labels(r["entries"]) == _labels(r32["entries"]), (shape, w, collapse, b)
            assert r["order"] == r32["order"] and r["best"] == r32["best"]


def test_extra_gpu_case_inputs():
    x, lm, w, W = F.constructed_case()
    for dtype in (np.float64, np.float32):
        entries, _, gaps = F.fused_nbest(x[0], 3, W, W, False, lm, w, 0.0, "per_beam", dtype)
        assert _labels(entries) == [[1], [1, 9]] and min(gaps["frame"], gaps["final"]) > MIN_GAP
    x, lm, w, bonus, W = F.wins_case()
    a, _, _ = F.fused_nbest(x[0], x.shape[1], W, W, False, lm, w, bonus, "per_beam")
    b, _, _ = F.fused_nbest(x[0], x.shape[1], W, W, False, lm, w, bonus, "per_beam", np.float32)
    assert _labels(a) == _labels(b)
    x, lm, w, bonus = F.fallback_case()
    _, T, _, W, N = F.FALLBACK_SHAPE
    a, _, gaps = F.fused_nbest(x[0], T, W, N, False, lm, w, bonus, "per_beam")
    b, _, _ = F.fused_nbest(x[0], T, W, N, False, lm, w, bonus, "per_beam", np.float32)
    assert _labels(a) == _labels(b) and min(gaps["frame"], gaps["final"]) > MIN_GAP


# ------------------------------------------------------------------------------ validation
def test_rescoring_fusion_validation():
    from scattennet_amd.nbest import BigramLM, Rescoring
    lm = BigramLM(np.zeros((4, 4), np.float32))
    assert Rescoring(3).fusion is False and "fusion=False" in repr(Rescoring(3))
    spec = Rescoring(3, lm, 0.5, 0.2, select="mbr", fusion=True)
    assert spec.fusion is True and "fusion=True" in repr(spec)
    assert Rescoring(3, None, 0.0, 0.2, fusion=True).fusion is True  # the bonus alone can be fused
    with pytest.raises(ValueError, match="nothing to fuse"):
        Rescoring(3, None, 0.5, 0.0, fusion=True)
    for bad in (1, 0, None, "yes", np.True_):
        with pytest.raises(ValueError, match="fusion must be a bool"):
            Rescoring(3, lm, 0.5, fusion=bad)


def test_fused_decode_argument_errors_come_before_any_device_call():
    import torch

    import scattennet_amd as S
    x = torch.zeros(2, 5, 4)
    lm = S.BigramLM(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="lm must be a BigramLM"):
        S.ctc_decode_fused_nbest_device(x, [5, 5], 3, np.zeros((4, 4)))
    with pytest.raises(ValueError, match="lm_weight must be finite"):
        S.ctc_decode_fused_nbest_device(x, [5, 5], 3, lm, float("nan"))
    with pytest.raises(ValueError, match="has 4 classes, the logits 6"):
        S.ctc_decode_fused_nbest_heads_device([torch.zeros(2, 5, 6)], [5, 5], 3, lm, 0.5)
    with pytest.raises(ValueError, match="nbest must lie"):
        S.ctc_decode_fused_nbest_device(x, [5, 5], 3, lm, nbest=4)
    with pytest.raises(RuntimeError, match="no CPU fallback|only on ROCm"):
        S.ctc_decode_fused_nbest_device(x, [5, 5], 3, lm, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback|only on ROCm"):
        S.ctc_decode_fused_nbest_heads_device([x, x], [5, 5], 3, lm, 0.5)
