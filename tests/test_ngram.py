"""The backoff n-gram gloss model on the host (scattennet_amd/ngram.py) and its float64 restatement
(tests/ngram_ref.py): the restatement against a brute-force enumeration on a hand-written model,
the estimator's normalisation, the ARPA text forms, the dense forms, the validation, and the
conditions on the GPU cases' inputs that tests/test_gpu_ngram.py relies on (tie margins, every
look-up outcome).  No GPU."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import nbest_ref as R
from tests import ngram_ref as NG

MIN_GAP = 1e-4  # the margin of tests/test_nbest.py


def _S():
    import scattennet_amd as S
    return S


# ------------------------------------------------------------------ the restatement itself
# three words a = 1, b = 2, c = 3 over C = 4; natural-log values chosen by hand
HAND = {"order": 3, "C": 4,
        "uni_lp": np.array([-1.0, -1.5, -2.0, -2.5], np.float32),
        "uni_bo": np.array([-0.25, -0.5, -0.75, -0.125], np.float32),
        "bi": {(0, 0): (-3.0, 0.0), (0, 1): (-0.5, -0.375), (1, 2): (-0.625, -0.875), (2, 1): (-1.25, -0.0625),
               (2, 0): (-0.75, 0.0), (1, 0): (-1.125, 0.0), (3, 3): (-2.25, -0.5)},
        "tri": {(0, 1, 2): -0.3125, (1, 2, 0): -0.4375, (2, 1, 2): -1.0625, (3, 3, 3): -0.1875}}


def _dense_hand(order):
    """p(w | u, v) of HAND for every cell, spelled out cell by cell without the recursion."""
    C = 4
    lp, bo, bi, tri = HAND["uni_lp"].astype(np.float64), HAND["uni_bo"].astype(np.float64), HAND["bi"], HAND["tri"]
    P2 = np.array([[bi[v, w][0] if (v, w) in bi else bo[v] + lp[w] for w in range(C)] for v in range(C)], np.float64)
    P3 = np.zeros((C, C, C))
    for u, v, w in itertools.product(range(C), repeat=3):
        if (u, v, w) in tri:
            P3[u, v, w] = tri[u, v, w]
        elif (u, v) in bi:
            P3[u, v, w] = bi[u, v][1] + P2[v, w]
        else:
            P3[u, v, w] = P2[v, w]
    return lp, P2, P3 if order == 3 else None


@pytest.mark.parametrize("order", [1, 2, 3])
def test_restatement_equals_the_enumeration(order):
    model = NG.truncated(HAND, order)
    lp, P2, P3 = _dense_hand(order)
    hyps = [()] + [h for n in (1, 2, 3, 4) for h in itertools.product((1, 2, 3), repeat=n)]
    assert () in hyps and (2,) in hyps
    for h in hyps:
        path = (0,) + h + (0,)
        want = 0.0
        for k in range(1, len(path)):
            if order == 1:
                want += lp[path[k]]
            elif order == 2 or k == 1:
                want += P2[path[k - 1], path[k]]
            else:
                want += P3[path[k - 2], path[k - 1], path[k]]
        assert NG.score(model, h) == pytest.approx(want, abs=1e-12), h
    # by hand: the empty hypothesis, one word, and one term of every kind
    assert NG.score(model, ()) == (-1.0 if order == 1 else -3.0)
    if order == 3:
        assert NG.score(model, (1,)) == -0.5 + (-0.375 + -1.125)  # p2(a | <s>), then bo(<s> a) + p2(</s> | a)
        assert NG.score(model, (1, 2)) == -0.5 + -0.3125 + -0.4375  # two stored trigrams
        # c after a: (0, 1) is stored, (1, 3) is not: bo(<s> a) + (uni_bo[a] + uni_lp[c]); then the context
        # (1, 3) is not stored and neither is (3, 0): uni_bo[c] + uni_lp[</s>]
        assert NG.score(model, (1, 3)) == -0.5 + (-0.375 + (-0.5 + -2.5)) + (-0.125 + -1.0)
    seen = dict.fromkeys(NG.OUTCOMES, 0)
    for h in hyps:
        NG.score(model, h, seen)
    assert all(seen[k] > 0 for k in NG.OUTCOMES) if order == 3 else seen["trigram hit"] == 0


def test_package_model_holds_the_hand_model():
    S = _S()
    lm = NG.build(S.NGramLM, HAND)
    assert (lm.order, lm.num_classes, lm.num_entries) == (3, 4, (4, 7, 4)) and lm.device.type == "cpu"
    assert "order=3" in repr(lm) and "C=4" in repr(lm)
    assert lm.bi_ptr.tolist() == [0, 2, 4, 6, 7] and lm.bi_tok.tolist() == [0, 1, 0, 2, 0, 1, 3]
    # trigram rows by bigram entry: (0,1) is entry 1, (1,2) entry 3, (2,1) entry 5, (3,3) entry 6
    assert lm.tri_ptr.tolist() == [0, 0, 1, 1, 2, 2, 3, 4] and lm.tri_tok.tolist() == [2, 0, 2, 3]
    assert lm.bigram_dict() == {k: (float(a), float(b)) for k, (a, b) in HAND["bi"].items()}
    assert lm.trigram_dict() == {k: float(v) for k, v in HAND["tri"].items()}
    assert all(t.dtype in (torch.float32, torch.int32) for t in lm.tensors.values())
    arrays = (np.array([0, 0, 1]), np.array([0, 1, 2]), np.array([-3.0, -0.5, -0.625]), np.array([0.0, -0.375, -0.875]))
    same = S.NGramLM(2, 4, HAND["uni_lp"], HAND["uni_bo"], arrays)
    assert same.bigram_dict() == {k: v for k, v in lm.bigram_dict().items() if k in ((0, 0), (0, 1), (1, 2))}
    moved = lm.to("cpu")
    assert moved is not lm and all(torch.equal(moved.tensors[k], lm.tensors[k]) for k in lm.tensors)


# ------------------------------------------------------------------ the estimator
SEQS = [[1, 2, 3], [1, 2], [2, 3, 3, 1], [], [4], [1, 2, 3, 4], [3, 1, 2]]


@pytest.mark.parametrize("order", [1, 2, 3])
def test_from_sequences_is_normalised_in_every_context(order):
    S = _S()
    C = 7  # classes 5 and 6 are never seen
    est = S.NGramLM.estimate(SEQS, C, order)
    assert est["uni_lp"].dtype == np.float64
    model = {"order": order, "C": C, "uni_lp": est["uni_lp"], "uni_bo": est["uni_bo"], "bi": est["bigrams"],
             "tri": est["trigrams"]}
    assert abs(np.exp(est["uni_lp"]).sum() - 1.0) <= 1e-9
    assert bool(est["bigrams"]) == (order >= 2) and bool(est["trigrams"]) == (order >= 3)
    if order >= 2:
        seen_ctx = sorted({v for v, _ in est["bigrams"]})
        assert 0 in seen_ctx and 5 not in seen_ctx  # the boundary context is seen, class 5 is not
        for v in seen_ctx + [5]:
            total = sum(math.exp(NG.p2(model, v, w)) for w in range(C))
            assert abs(total - 1.0) <= 1e-9, (v, total)
    if order == 3:
        seen_ctx = sorted({(u, v) for u, v, _ in est["trigrams"]})
        assert (0, 1) in seen_ctx and (5, 1) not in seen_ctx
        for u, v in seen_ctx + [(5, 1), (2, 5)]:  # every seen context, the boundary ones among them, and unseen ones
            total = sum(math.exp(NG.p3(model, u, v, w)) for w in range(C))
            assert abs(total - 1.0) <= 1e-9, (u, v, total)
    lm = S.NGramLM.from_sequences(SEQS, C, order)
    assert lm.order == order and lm.num_entries == (C, len(est["bigrams"]), len(est["trigrams"]))
    assert np.array_equal(lm.uni_lp.numpy(), est["uni_lp"].astype(np.float32))
    # p1 by hand: N = 24 tokens with </s>, add-1 over 7 classes
    assert est["uni_lp"][1] == pytest.approx(math.log((5 + 1) / (24 + 7)))
    assert est["uni_lp"][0] == pytest.approx(math.log((7 + 1) / (24 + 7)))


def test_from_sequences_rejects_bad_arguments():
    S = _S()
    for kw in (dict(order=4), dict(order=0), dict(discount=0.0), dict(discount=1.0), dict(add_k=0.0),
               dict(add_k=float("nan"))):
        with pytest.raises(ValueError):
            S.NGramLM.from_sequences(SEQS, 7, **kw)
    with pytest.raises(ValueError):
        S.NGramLM.from_sequences([[0, 1]], 7)
    with pytest.raises(ValueError):
        S.NGramLM.from_sequences([[7]], 7)


# ------------------------------------------------------------------ ARPA
VOCAB = {"A": 1, "B": 2, "C": 3, "D": 4, "E": 5, "F": 6}


@pytest.mark.parametrize("order", [1, 2, 3])
def test_arpa_round_trip(order):
    S = _S()
    lm = S.NGramLM.from_sequences(SEQS, 7, order)
    text = lm.to_arpa(VOCAB)
    assert text.startswith("\\data\\\nngram 1=8\n") and text.rstrip().endswith("\\end\\")
    back = S.NGramLM.from_arpa(text, VOCAB)
    assert back.order == order and back.num_classes == 7 and back.skipped == 0
    for k, a in lm.tensors.items():
        b = back.tensors[k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        if a.dtype == torch.int32:
            assert torch.equal(a, b), k
        else:  # 9 significant digits of log10: within one fp32 rounding
            assert bool(((a - b).abs() <= 2.0 ** -22 * a.abs()).all()), k


ARPA = """\\data\\
ngram 1=6
ngram 2=5
ngram 3=3

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.5\tHELLO\t-0.25
-0.75\tWORLD\t-0.125
-2.0\tOOV\t-0.1
-3.0\t<unk>

\\2-grams:
-0.25\t<s> HELLO\t-0.0625
-0.5\tHELLO WORLD\t-0.03125
-0.125\tWORLD </s>
-1.5\tHELLO OOV\t-0.2
-1.25\t</s> HELLO

\\3-grams:
-0.0625\t<s> HELLO WORLD
-0.03125\tHELLO WORLD </s>
-0.7\tHELLO OOV WORLD

\\end\\
"""


def test_inline_arpa_text_loads_to_the_expected_arrays(tmp_path):
    S = _S()
    vocab = {"HELLO": 1, "WORLD": 2, "NEVER": 3}
    ln10 = math.log(10.0)
    for src in (ARPA, tmp_path / "toy.arpa"):
        if not isinstance(src, str):
            src.write_text(ARPA)
        lm = S.NGramLM.from_arpa(src, vocab)
        assert (lm.order, lm.num_classes, lm.num_entries) == (3, 4, (4, 3, 2))
        # skipped: OOV, <unk>, HELLO OOV, </s> HELLO (no sentence has </s> as a context), HELLO OOV WORLD
        assert lm.skipped == 5
        f32 = np.float32
        # class 3 has no unigram: the <unk> value and backoff weight 0
        assert np.array_equal(lm.uni_lp.numpy(), (np.array([-1.0, -0.5, -0.75, -3.0]) * ln10).astype(f32))
        assert np.array_equal(lm.uni_bo.numpy(), (np.array([-0.5, -0.25, -0.125, 0.0]) * ln10).astype(f32))
        assert lm.bi_ptr.tolist() == [0, 1, 2, 3, 3] and lm.bi_tok.tolist() == [1, 2, 0]
        assert np.array_equal(lm.bi_lp.numpy(), (np.array([-0.25, -0.5, -0.125]) * ln10).astype(f32))
        assert np.array_equal(lm.bi_bo.numpy(), (np.array([-0.0625, -0.03125, 0.0]) * ln10).astype(f32))
        assert lm.tri_ptr.tolist() == [0, 1, 2, 2] and lm.tri_tok.tolist() == [2, 0]
        assert np.array_equal(lm.tri_lp.numpy(), (np.array([-0.0625, -0.03125]) * ln10).astype(f32))
    with pytest.raises(ValueError, match="order 4"):
        S.NGramLM.from_arpa(ARPA.replace("\\end\\", "\\4-grams:\n-1.0\tHELLO WORLD HELLO WORLD\n\n\\end\\"), vocab)
    with pytest.raises(ValueError):
        S.NGramLM.from_arpa(ARPA, {"HELLO": 0})
    with pytest.raises(ValueError):
        S.NGramLM.from_sequences(SEQS, 7, 2).to_arpa({"A": 1})


# ------------------------------------------------------------------ the dense forms
def test_from_bigram_to_bigram_is_the_identity_on_the_bits():
    S = _S()
    table = R.random_lm(33)
    dense = S.BigramLM(table)
    sparse = S.NGramLM.from_bigram(dense)
    assert sparse.order == 2 and sparse.num_entries == (33, 33 * 33, 0)
    back = sparse.to_bigram()
    assert isinstance(back, S.BigramLM) and np.array_equal(back.table.numpy().view(np.int32), table.view(np.int32))


def test_to_bigram_holds_the_backoff_sums_in_fp32():
    S = _S()
    model = NG.truncated(NG.random_ngram(12, 3, 5), 2)
    table = NG.build(S.NGramLM, model).to_bigram().table.numpy()
    for v in range(12):
        for w in range(12):
            want = model["bi"][v, w][0] if (v, w) in model["bi"] else model["uni_bo"][v] + model["uni_lp"][w]
            assert table[v, w] == np.float32(want) and table.dtype == np.float32, (v, w)
    uni = NG.build(S.NGramLM, NG.truncated(model, 1)).to_bigram().table.numpy()
    assert all(np.array_equal(row, model["uni_lp"]) for row in uni)
    with pytest.raises(ValueError, match="order 1 or 2"):
        NG.build(S.NGramLM, HAND).to_bigram()


# ------------------------------------------------------------------ validation
def test_constructor_validation():
    S = _S()
    lp, bo = HAND["uni_lp"], HAND["uni_bo"]
    ok = dict(bigrams={(0, 1): (-1.0, -0.5), (1, 2): (-1.0, 0.0)}, trigrams={(0, 1, 2): -1.0})
    S.NGramLM(3, 4, lp, bo, **ok)
    bad = [
        dict(order=0), dict(order=4), dict(order=True), dict(num_classes=0), dict(num_classes=8193),
        dict(uni_lp=lp[:3]), dict(uni_lp=np.array([0.0, np.inf, 0.0, 0.0])), dict(uni_bo=np.array([0.0, np.nan, 0, 0])),
        dict(bigrams={(0, 1): (float("inf"), 0.0)}, trigrams=None),          # a value that is not finite
        dict(bigrams={(0, 4): -1.0}, trigrams=None), dict(bigrams={(-1, 1): -1.0}, trigrams=None),  # tokens
        dict(trigrams={(0, 1, 4): -1.0}),
        dict(bigrams={(0, 1): -1.0, (1, 0): -1.0}, trigrams={(1, 0, 1): -1.0}),  # the boundary inside a trigram
        dict(trigrams={(0, 2, 1): -1.0}),                                    # (0, 2) is not a stored bigram
        dict(trigrams={(2, 1, 1): -1.0}),
        dict(bigrams=(np.array([1, 0]), np.array([2, 1]), np.array([-1.0, -1.0])), trigrams=None),  # rows not sorted
        dict(bigrams=(np.array([0, 0]), np.array([1, 1]), np.array([-1.0, -1.0])), trigrams=None),  # a row twice
        dict(trigrams=(np.array([0, 0]), np.array([1, 1]), np.array([2, 2]), np.array([-1.0, -1.0]))),
        dict(bigrams={(0, 1, 2): -1.0}, trigrams=None), dict(bigrams=(np.array([0]),), trigrams=None),
        dict(order=2), dict(order=1, trigrams=None),                         # n-grams above the order
    ]
    for change in bad:
        kw = dict(order=3, num_classes=4, uni_lp=lp, uni_bo=bo, **ok)
        kw.update(change)
        with pytest.raises(ValueError):
            S.NGramLM(**kw)


def test_where_a_model_is_accepted_and_where_it_is_not():
    S = _S()
    lm = NG.build(S.NGramLM, HAND)
    spec = S.Rescoring(3, lm, 0.5, 0.1, select="mbr")
    assert spec.lm is lm and "NGramLM" in repr(spec)
    spec.check(5, 4, 16, "test")
    with pytest.raises(ValueError, match="classes"):
        spec.check(5, 6, 16, "test")
    m = S.MWER(1.0, lm=lm, lm_weight=0.5)
    assert m.lm is lm
    for make in (lambda: S.Rescoring(3, lm, 0.5, fusion=True), lambda: S.MWER(1.0, lm=lm, lm_weight=0.5, fusion=True)):
        with pytest.raises(ValueError, match=r"BigramLM.*to_bigram\(\)"):
            make()
    x = torch.zeros(2, 6, 4)
    il = torch.tensor([6, 6])
    with pytest.raises(ValueError, match=r"BigramLM.*to_bigram\(\)"):
        S.ctc_decode_fused_nbest_device(x, il, 4, lm, 0.5)
    with pytest.raises(ValueError, match=r"BigramLM.*to_bigram\(\)"):
        S.ctc_decode_fused_nbest_heads_device([x, x], il, 4, lm, 0.5)
    with pytest.raises(ValueError, match=r"BigramLM.*to_bigram\(\)"):
        S.mwer_loss(x, il, torch.tensor([[1], [2]]), torch.tensor([1, 1]), lm=lm, lm_weight=0.5, fusion=True)
    with pytest.raises(ValueError, match="classes"):
        S.mwer_loss(torch.zeros(2, 6, 5), il, torch.tensor([[1], [2]]), torch.tensor([1, 1]), lm=lm, lm_weight=0.5)
    nb = S.NBest(torch.zeros(2, 3, 6, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3),
                 torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="ROCm"):  # there is no host path for the sparse model either
        S.rescore_nbest_device(nb, lm, 0.5)
    with pytest.raises(ValueError, match="NGramLM"):
        S.rescore_nbest_device(nb, object())


# ------------------------------------------------------------------ the GPU cases' inputs
@pytest.mark.parametrize("shape", NG.SHAPES, ids=["B%d_T%d_C%d_W%d_N%d" % s for s in NG.SHAPES])
def test_gpu_cases_keep_their_margins_and_meet_every_outcome(shape):
    assert shape in R.CASES
    clips, seen = NG.case_ref(shape)
    gap = min(min(c["gaps"].values()) for c in clips)
    print(shape, "min gap %.3e" % gap, seen)
    assert gap >= MIN_GAP, [c["gaps"] for c in clips]
    assert all(seen[k] >= 1 for k in NG.OUTCOMES), seen
