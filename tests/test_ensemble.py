"""Head ensembling and the label-free recognition step, host side (scattennet_amd/ensemble.py,
recognize.py; sca_ensemble_log_probs of include/scatten.h): the float64 restatement of
tests/ensemble_ref.py against torch's float64 composition and against its own properties,
every argument error before any device call, and the entry point's declaration.  CPU only."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import decode_ref as D
from tests import ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (5, 2, 9, 33), (8, 1, 3, 1124)]  # (G, B, T, C)
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
MIN_GAP = 1e-4  # tests/test_decode.py
ALL = ("alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits")


def _torch_composition(xs, weights, mode):
    """What the fused call replaces, in float64."""
    w = torch.tensor(R.normalised(weights, len(xs)))
    lps = [torch.log_softmax(torch.from_numpy(x).double(), -1) for x in xs]
    if mode == "prob":
        return torch.logsumexp(torch.stack([lp + torch.log(w[g]) for g, lp in enumerate(lps)]), 0).numpy()
    return torch.log_softmax(sum(w[g] * lp for g, lp in enumerate(lps)), -1).numpy()


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_the_torch_composition(shape, mode):
    G = shape[0]
    xs = R.case(*shape, clamp_rows=G >= 2 and shape[1] * shape[2] >= 3)
    for weights in (None, R.cycled_weights(G)):
        got = R.ensemble(xs, weights, mode)
        want = _torch_composition(xs, weights, mode)
        assert got.shape == xs[0].shape and np.isfinite(got).all()
        assert float(np.abs(got - want).max()) <= 1e-12 * max(1.0, float(np.abs(want).max())), (mode, weights)
        # normalised log-probabilities
        assert float(np.abs(np.exp(got).sum(-1) - 1.0).max()) <= 1e-12


@pytest.mark.parametrize("mode", R.MODES)
def test_one_member_is_log_softmax_and_prob_ignores_the_weights_scale(mode):
    xs = R.case(3, 2, 7, 70)
    one = R.ensemble(xs[:1], [2.5], mode)
    assert float(np.abs(one - D.log_softmax(xs[0])).max()) <= 1e-12
    w = np.array([0.2, 1.0, 3.0])
    a, b = R.ensemble(xs, w, mode), R.ensemble(xs, 37.5 * w, mode)
    assert float(np.abs(a - b).max()) <= 1e-12
    assert float(np.abs(R.ensemble(xs, None, mode) - R.ensemble(xs, [4.0] * 3, mode)).max()) <= 1e-12


def test_hand_case():
    """Posteriors (0.9, 0.1) and (0.5, 0.5): the arithmetic mean is (0.7, 0.3), the geometric one
    (sqrt 0.45, sqrt 0.05) normalised."""
    xs = [np.log(np.array([[[0.9, 0.1]]])) + 3.0, np.log(np.array([[[0.5, 0.5]]])) - 1.0]  # any shift per row
    assert np.allclose(np.exp(R.ensemble(xs, None, "prob")), [[[0.7, 0.3]]], rtol=0, atol=1e-15)
    g = np.sqrt(np.array([0.45, 0.05]))
    assert np.allclose(np.exp(R.ensemble(xs, None, "logprob")), [[g / g.sum()]], rtol=0, atol=1e-15)
    # weights 3 : 1
    assert np.allclose(np.exp(R.ensemble(xs, [3, 1], "prob")), [[[0.8, 0.2]]], rtol=0, atol=1e-15)


def test_clamped_logits_neither_overflow_nor_vanish():
    xs = R.case(2, 1, 3, 6, clamp_rows=True)
    for mode in R.MODES:
        out = R.ensemble(xs, None, mode)
        assert np.isfinite(out).all()
    p = R.ensemble(xs, None, "prob")
    assert abs(p[0, 0, 1] - math.log(0.5)) < 1e-6  # one member is sure of class 1, the other excludes it
    assert abs(p[0, 2, 5]) < 1e-12 and p[0, 2, 0] < -50  # every member at -50 except one class


def test_beam_case_is_away_from_ties():
    """The inputs of the GPU beam test (tests/test_gpu_ensemble.py): the restatement's decode of
    the float64 ensemble keeps its tie margins, in both modes, for every clip."""
    xs = R.beam_case()
    for mode in R.MODES:
        e = R.ensemble(xs, None, mode)
        hyps, _, frame_gap, final_gap = D.beam_search_batch(e, R.BEAM_LENS, R.BEAM_WIDTH, True)
        print(mode, hyps, frame_gap, final_gap)
        assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP, (mode, frame_gap, final_gap)
        assert all(len(h) > 0 for h in hyps)


# ---------------------------------------------------------------------------- the entry point
def test_entry_point_is_declared_exported_and_bound():
    from scattennet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)
    name = "sca_ensemble_log_probs"
    assert re.search(r"^\s*int\s+%s\s*\(" % name, src, flags=re.M)
    assert name in _lib.EXPORTS
    nargs = len(re.search(r"%s\s*\((.*?)\)" % name, src, flags=re.S).group(1).split(","))
    assert len(_lib.EXPORTS[name][0]) == nargs == 9
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert ctypes.sizeof(_lib.EnsembleWeights) == 4 * _lib.EVAL_MAX_HEADS
    assert "ensemble.hip" in open(os.path.join(ROOT, "scattennet_amd", "csrc", "Makefile")).read()
    assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_c_argument_validation_makes_no_gpu_call():
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    fn = lib.sca_ensemble_log_probs
    fn.argtypes, fn.restype = L.EXPORTS["sca_ensemble_log_probs"]
    hx, wx = L.DecodeHeads(), L.EnsembleWeights()
    for g in range(8):
        hx.logits[g] = 0x1000
        wx.w[g] = 1.0
    out = ctypes.c_void_p(0x2000)

    def call(G=2, mode=0, B=2, T=3, C=5, heads=hx, weights=wx, out=out):
        return fn(None if heads is None else ctypes.byref(heads), G, None if weights is None else ctypes.byref(weights),
                  mode, B, T, C, out, None)
    assert call(G=0) == 1 and call(G=9) == 1 and call(mode=2) == 1 and call(mode=-1) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(C=0) == 1
    assert call(heads=None) == 1 and call(weights=None) == 1 and call(out=None) == 1
    assert call(out=ctypes.c_void_p(0x1000)) == 1  # in place
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000
    assert call(heads=hole) == 1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = L.EnsembleWeights()
        w.w[0], w.w[1] = 1.0, bad
        assert call(weights=w) == 1, bad
    with pytest.raises(ValueError, match="sca_ensemble_log_probs"):
        L.check(call(G=9), "sca_ensemble_log_probs")


# ------------------------------------------------------------------------ Python validation
def test_ensemble_log_probs_validation_comes_before_the_device():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.ensemble_log_probs([])
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.ensemble_log_probs([x] * 9)
    with pytest.raises(ValueError, match="same shape"):
        S.ensemble_log_probs([x, torch.randn(2, 8, 13)])
    with pytest.raises(ValueError, match="same shape"):
        S.ensemble_log_probs([x, x.double()])
    with pytest.raises(ValueError, match="empty"):
        S.ensemble_log_probs([torch.randn(0, 8, 12)])
    with pytest.raises(RuntimeError, match="batch-major"):
        S.ensemble_log_probs([torch.randn(8, 12)])
    with pytest.raises(ValueError, match="mode"):
        S.ensemble_log_probs([x, x], mode="mean")
    for bad in ([1.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")], [1.0, "a"], 3.0,
                [1.0, 1e-60]):
        with pytest.raises(ValueError, match="weights"):
            S.ensemble_log_probs([x, x], weights=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ensemble_log_probs([x, x], weights=[1, 2], mode="logprob")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ensemble_log_probs([x.half()])


def test_ensemble_spec_errors():
    import scattennet_amd as S
    spec = S.EnsembleSpec(ALL, weights=[1, 1, 1, 1, 4], mode="logprob")
    assert spec.members == ALL and spec.mode == "logprob" and abs(sum(spec.weights) - 1.0) < 1e-15
    assert S.EnsembleSpec(["left"]).weights is None
    with pytest.raises(ValueError, match="unknown member"):
        S.EnsembleSpec(("left", "gloss_logits"))
    with pytest.raises(ValueError, match="distinct"):
        S.EnsembleSpec(("left", "left"))
    with pytest.raises(ValueError, match="distinct"):
        S.EnsembleSpec(())
    with pytest.raises(ValueError, match="string"):
        S.EnsembleSpec("left")
    with pytest.raises(ValueError, match="mode"):
        S.EnsembleSpec(ALL, mode="geometric")
    with pytest.raises(ValueError, match="weights"):
        S.EnsembleSpec(ALL, weights=[1, 2])
    with pytest.raises(ValueError, match="weights"):
        S.EnsembleSpec(("left", "right"), weights=[1, 0])


class _Model:
    """Enough of MSCA_Net for the constructors: cfg, the distillation students, a parameter."""

    def __init__(self, blocks=(64,), maxpos=4096):
        self.cfg = {"residual_blocks": list(blocks), "max_position_embeddings": maxpos}
        self._p = torch.nn.Parameter(torch.zeros(1))

    def _students(self):
        return ["left", "right", "body"]

    def parameters(self):
        return iter([self._p])


def _bad_ensembles(S):
    spec = S.EnsembleSpec(ALL)
    return [({"ensemble": spec}, "must contain 'gloss_logits'"),
            ({"fuse_coord_gloss_logits": spec}, "own logit keys"),
            ({"ensemble_gloss_logits": ALL}, "must be an EnsembleSpec"),
            ([("ensemble_gloss_logits", spec)], "must be a dict"),
            ({"e%d_gloss_logits" % i: spec for i in range(7)}, "more than the 8")]


def test_eval_state_ensembles_errors_and_layout():
    import scattennet_amd as S
    m = _Model()
    for bad, msg in _bad_ensembles(S):
        with pytest.raises(ValueError, match=msg):
            S.EvalState(m, ensembles=bad)
        with pytest.raises(ValueError, match=msg):
            S.BucketedEvalStep(m, 3, (64,), 8, ensembles=bad)
    spec = S.EnsembleSpec(ALL)
    six = {"e%d_gloss_logits" % i: spec for i in range(6)}
    assert len(S.EvalState(m, ensembles=six).keys) == 8  # 2 heads + 6 ensembles fit
    with pytest.raises(ValueError, match="more than the 8"):
        S.EvalState(m, heads=ALL, ensembles={k: spec for k in list(six)[:4]})
    st = S.EvalState(m, capacity=4, log_width=16, align=True, ensembles={"ensemble_gloss_logits": spec})
    assert st.heads == ("alignment_gloss_logits", "fuse_coord_gloss_logits")
    assert st.keys == st.heads + ("ensemble_gloss_logits",)
    assert st.hyp_log.shape == (4, 3, 16) and st.span_log.shape == (4, 3, 16, 2) and st.score_log.shape == (4, 3)
    plain = S.EvalState(m, capacity=4, log_width=16)
    assert plain.keys == plain.heads and plain.ensembles == {} and plain.hyp_log.shape == (4, 2, 16)
    # read() reports the ensemble under its logits_name and includes it in the minimum
    from scattennet_amd import evaluate as E
    raw = {"cursor": 0, "steps": 1, "overflow": 0, "first_flagged": 0, "flags": [0] * 64,
           "totals": np.array([[1, 0, 1, 10], [0, 1, 0, 10], [0, 0, 0, 10]] + [[0] * 4] * 5), "loss_sum": np.ones(11)}
    got = E.results_from_state(raw, st.keys, st.loss_names, st.flag_names)
    assert got["alignment_wer"] == 20.0 and got["fuse_coord_wer"] == 10.0
    assert got["ensemble_wer"] == 10.0 and got["wer"] == 10.0  # no errors: a zero total counts as 1


def test_bucketed_recognizer_constructor_errors():
    import scattennet_amd as S
    m = _Model()
    for bad, msg in _bad_ensembles(S):
        with pytest.raises(ValueError, match=msg):
            S.BucketedRecognizer(m, 3, (64,), ensembles=bad)
    with pytest.raises(ValueError, match="multiple of"):
        S.BucketedRecognizer(m, 3, (33,))
    with pytest.raises(ValueError, match="distinct and non-empty"):
        S.BucketedRecognizer(m, 3, ())
    with pytest.raises(ValueError, match="max_position_embeddings"):
        S.BucketedRecognizer(m, 3, (8192,))
    with pytest.raises(ValueError, match="positive"):
        S.BucketedRecognizer(m, 0, (64,))
    with pytest.raises(ValueError, match="unknown head"):
        S.BucketedRecognizer(m, 3, (64,), heads=("gloss_logits",))
    with pytest.raises(ValueError, match="distinct"):
        S.BucketedRecognizer(m, 3, (64,), heads=("left", "left"))
    with pytest.raises(ValueError, match="pooled frames"):
        S.BucketedRecognizer(m, 3, (64, 2048))  # 2048 >> 1 = 1024 labels to align
    rec = S.BucketedRecognizer(m, 3, (2048, 64), align=False, ensembles={"ensemble_gloss_logits": S.EnsembleSpec(ALL)})
    assert rec.frame_buckets == (64, 2048) and rec.graphs_captured == 0 and rec.eager_fallbacks == 0
    assert rec.heads == ("alignment_gloss_logits", "fuse_coord_gloss_logits")
    with pytest.raises(ValueError, match="unknown head"):
        S.recognize_step(m, {}, heads=("nope",))
    with pytest.raises(ValueError, match="must contain"):
        S.recognize_step(m, {}, ensembles={"ensemble": S.EnsembleSpec(ALL)})


def test_predict_flag_names_and_recognition_read():
    import scattennet_amd as S
    from scattennet_amd import model as M
    assert M.predict_flag_names() == M.flag_names()[:10] == M.flag_names(("left", "right", "body"))[:10]
    assert M.predict_flag_names()[0] == "keypoints" and M.predict_flag_names()[5:] == list(ALL)
    assert hasattr(S.MSCA_Net, "predict")
    # Recognition.read on host tensors: the packing, the flags and the lists
    keys = ("fuse_coord_gloss_logits", "ensemble_gloss_logits")
    out = {"finite_flags": torch.zeros(10, dtype=torch.int32),
           "tokens": torch.tensor([[[5, 7, 0], [2, 0, 0]], [[5, 0, 0], [0, 0, 0]]], dtype=torch.int32),
           "lengths": torch.tensor([[2, 1], [1, 0]], dtype=torch.int32),
           "spans": torch.tensor([[[[0, 1], [2, 3], [0, 0]], [[1, 2], [0, 0], [0, 0]]],
                                  [[[0, 3], [0, 0], [0, 0]], [[0, 0], [0, 0], [0, 0]]]], dtype=torch.int32),
           "conf": torch.tensor([[[0.5, 0.25, 0], [1.0, 0, 0]], [[0.75, 0, 0], [0, 0, 0]]]),
           "align_scores": torch.tensor([[-1.0, -2.0], [-0.5, 0.0]])}
    rec = S.Recognition(out, keys, True, 4)
    assert rec.read() == [{"fuse_coord_": [(5, 0, 4, 0.5), (7, 8, 12, 0.25)], "ensemble_": [(5, 0, 12, 0.75)]},
                          {"fuse_coord_": [(2, 4, 8, 1.0)], "ensemble_": []}]
    assert rec.read(frame_scale=1)[0]["fuse_coord_"] == [(5, 0, 1, 0.5), (7, 2, 3, 0.25)]
    plain = S.Recognition({k: out[k] for k in ("finite_flags", "tokens", "lengths")}, keys, False, 4)
    assert plain.read() == [{"fuse_coord_": [5, 7], "ensemble_": [5]}, {"fuse_coord_": [2], "ensemble_": []}]
    out["finite_flags"][0] = 1
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        rec.read()
    out["finite_flags"][0], out["finite_flags"][9] = 0, 2
    with pytest.raises(ValueError, match="^inf in fuse_coord_gloss_logits$"):
        rec.read()
