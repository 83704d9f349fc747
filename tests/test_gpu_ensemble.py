"""Head ensembling and the label-free recognition step on the MI355X
(scattennet_amd/ensemble.py, recognize.py; csrc/ensemble.hip: sca_ensemble_log_probs) against the
float64 restatement of tests/ensemble_ref.py, through the decoders, bitwise across eager /
captured / reduced-precision forms, and inside the evaluation and recognition steps on the
reference's fixture.

Parity bound: |out - ref| <= 1e-3 max(1, |ref|) element-wise, the project's bound, over every
element.  Measured maximum of |out - ref| / max(1, |ref|) over all parity cases on one MI355X:
7.7e-7."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import decode_ref as D
from tests import ensemble_ref as R
from tests.golden_util import load

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's relative bound
# (G, B, T, C): C below a wave; C % 4 != 0 (misaligned rows); C % 64 != 0; 1, 3, 14, 15 rows (not a
# multiple of the four rows per workgroup); G = 1 and 8; the evaluation shape
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (3, 2, 7, 70), (5, 3, 5, 33), (8, 1, 3, 1124), (2, 8, 64, 1124)]
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
CLAMPED = {(3, 2, 7, 70), (2, 8, 64, 1124)}  # these also hold the +-50 rows (ensemble_ref.case)
ALL = ("alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits")
ENS = "ensemble_gloss_logits"


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(inputs, {(weighted, mode): float64 restatement}), computed once per shape."""
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    refs = {(wt, mode): R.ensemble(xs, R.cycled_weights(shape[0]) if wt else None, mode)
            for wt in (False, True) for mode in R.MODES}
    return xs, refs


def _err(out, ref):
    return float((np.abs(out.astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max())


# ------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ensemble_against_the_restatement(shape):
    import scattennet_amd as S
    dev = _dev()
    xs, refs = _case(shape)
    xd = [torch.from_numpy(x).to(dev) for x in xs]
    for (weighted, mode), ref in refs.items():
        w = R.cycled_weights(shape[0]) if weighted else None
        out = S.ensemble_log_probs(xd, w, mode)
        assert out.shape == xd[0].shape and out.dtype == torch.float32 and not out.requires_grad
        got = out.cpu().numpy()
        err = _err(got, ref)
        print(f"{IDS[SHAPES.index(shape)]} {mode} weighted={weighted}: max err {err:.3e}")
        assert np.isfinite(got).all(), (mode, weighted)
        assert err <= TOL, (mode, weighted, err)  # every element
        assert float(np.abs(np.exp(got.astype(np.float64)).sum(-1) - 1.0).max()) <= TOL


def test_one_member_equals_log_softmax():
    import scattennet_amd as S
    dev = _dev()
    for shape in ((1, 1, 1, 2), (1, 3, 5, 33), (1, 2, 7, 1124)):
        x = torch.from_numpy(R.case(*shape)[0]).to(dev)
        want = torch.log_softmax(x.double(), -1).cpu().numpy()
        for mode in R.MODES:
            got = S.ensemble_log_probs([x], [2.5], mode).cpu().numpy()
            assert _err(got, want) <= TOL, (shape, mode)
            assert _err(got, torch.log_softmax(x, -1).cpu().numpy().astype(np.float64)) <= TOL, (shape, mode)


# ------------------------------------------------------------------ 2: through the decoders
def test_the_ensemble_finds_what_no_member_does():
    import scattennet_amd as S
    dev = _dev()
    a, b = np.zeros((1, 8, 6), np.float32), np.zeros((1, 8, 6), np.float32)
    for t, c in enumerate((1, 0, 2, 0)):
        a[0, t, c] = 10.0
    for t, c in enumerate((3, 0, 4, 0)):
        b[0, 4 + t, c] = 10.0
    il = torch.tensor([8])

    def greedy(x):
        tokens, lengths, _ = S.ctc_decode_heads_device([x], il, beam_size=0)
        return tokens[0, 0, :int(lengths[0, 0])].tolist()
    ad, bd = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    assert greedy(ad) == [1, 2] and greedy(bd) == [3, 4]
    for mode in R.MODES:
        ref = np.exp(R.ensemble([a, b], None, mode))[0]
        top = np.sort(ref, axis=-1)
        assert (top[:, -1] > 0.5).all() and (top[:, -2] <= 0.1).all()  # no tie is near (on the inputs)
        e = S.ensemble_log_probs([ad, bd], None, mode)
        assert greedy(e) == [1, 2, 3, 4], mode


def test_beam_decode_of_the_ensemble_equals_the_restatement():
    import scattennet_amd as S
    dev = _dev()
    xs = R.beam_case()  # its tie margins are asserted on the CPU, tests/test_ensemble.py
    xd = [torch.from_numpy(x).to(dev) for x in xs]
    il = torch.tensor(R.BEAM_LENS)
    for mode in R.MODES:
        want, _, frame_gap, final_gap = D.beam_search_batch(R.ensemble(xs, None, mode), R.BEAM_LENS, R.BEAM_WIDTH, True)
        assert frame_gap >= 1e-4 and final_gap >= 1e-4
        tokens, lengths, _ = S.ctc_decode_device(S.ensemble_log_probs(xd, None, mode), il, beam_size=R.BEAM_WIDTH)
        tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
        for b in range(len(want)):  # every clip
            assert lengths[b] == len(want[b]) and tokens[b, :lengths[b]].tolist() == want[b], (mode, b)
            assert not tokens[b, lengths[b]:].any()


# ------------------------------------------------------------------ 3: bitwise forms
def test_captured_ensemble_replayed_on_refilled_inputs_equals_eager():
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs = [torch.from_numpy(x).to(dev) for x in R.case(*shape)]
    w = R.cycled_weights(3)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for mode in R.MODES:
            S.ensemble_log_probs(xs, w, mode)  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = [S.ensemble_log_probs(xs, w, mode) for mode in R.MODES]
    graph.replay()
    torch.cuda.synchronize()
    for mode, out in zip(R.MODES, outs):
        assert torch.equal(_bits(out), _bits(S.ensemble_log_probs(xs, w, mode))), mode
    for g, x in enumerate(R.case(*shape, seed=5)):  # refill the static inputs
        xs[g].copy_(torch.from_numpy(x))
    graph.replay()
    torch.cuda.synchronize()
    for mode, out in zip(R.MODES, outs):
        eager = S.ensemble_log_probs(xs, w, mode)
        assert torch.equal(_bits(out), _bits(eager)), mode
        # a row's result does not depend on the rows beside it
        one = S.ensemble_log_probs([x[1:, 2:3].contiguous() for x in xs], w, mode)
        assert torch.equal(_bits(one), _bits(eager[1:, 2:3])), mode


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_reduced_precision_logits_take_the_fp32_path(dtype):
    import scattennet_amd as S
    dev = _dev()
    low = [torch.from_numpy(x).to(dev).to(dtype) for x in R.case(3, 2, 7, 70)]
    for mode in R.MODES:
        got = S.ensemble_log_probs(low, [1, 2, 3], mode)
        want = S.ensemble_log_probs([x.float() for x in low], [1, 2, 3], mode)
        assert got.dtype == dtype and torch.equal(got, want.to(dtype)), mode


# ------------------------------------------------------------------ 4: the evaluation step
@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


@pytest.fixture(scope="module")
def model(fx):
    """The fixture model, built as tests/test_gpu_align.py builds it; eval mode, never modified."""
    import scattennet_amd as S
    dev = _dev()
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


def _src(fx, dev):
    return {k: v.to(dev) for k, v in fx["in"].items()}


def _spec():
    import scattennet_amd as S
    return {ENS: S.EnsembleSpec(ALL)}


def test_eval_step_with_an_ensemble_of_all_heads(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    plain_state = S.EvalState(model, capacity=3, log_width=13, align=True)
    plain = S.eval_step(model, src, plain_state)
    state = S.EvalState(model, capacity=3, log_width=13, align=True, ensembles=_spec())
    out = S.eval_step(model, src, state)
    assert ENS not in plain and out[ENS].shape == out["left"].shape
    assert out["tokens"].shape == (3, 3, 13) and out["counts"].shape == (3, 3, 4) and out["spans"].shape == (3, 3, 13, 2)
    # the two default heads: bitwise the state without ensembles
    for k in ("tokens", "lengths", "counts", "spans"):
        assert torch.equal(out[k][:2], plain[k]), k
    assert torch.equal(_bits(out["conf"][:2]), _bits(plain["conf"]))
    assert torch.equal(_bits(out["finite_report"]), _bits(plain["finite_report"]))
    ra, rb = state.raw(), plain_state.raw()
    assert ra["totals"][:2].tolist() == rb["totals"][:2].tolist() and not rb["totals"][2:].any()
    assert ra["loss_sum"].tolist() == rb["loss_sum"].tolist() and ra["flags"] == rb["flags"]
    hyps, plain_hyps = state.hypotheses(), plain_state.hypotheses()
    assert [{k: h[k] for k in ("alignment_", "fuse_coord_")} for h in hyps] == plain_hyps
    assert sorted(hyps[0]) == ["alignment_", "ensemble_", "fuse_coord_"]
    # the ensemble: the op on the step's own logits, decoded, scored and aligned like a head
    e = S.ensemble_log_probs([out[k] for k in ALL])
    assert torch.equal(_bits(out[ENS]), _bits(e))
    t, n, _ = S.ctc_decode_device(e, out["input_lengths"], beam_size=5)
    assert torch.equal(out["tokens"][2], t) and torch.equal(out["lengths"][2], n)
    tn, nn_ = t.cpu().numpy(), n.cpu().numpy()
    assert [h["ensemble_"] for h in hyps] == [tn[b, :nn_[b]].tolist() for b in range(3)]
    c = S.wer_counts(src["gloss_labels"].to(torch.int32), src["gloss_lengths"], t, n)
    assert torch.equal(out["counts"][2], c) and ra["totals"][2].tolist() == c.sum(0).tolist()
    res = S.ctc_align_device(e, out["input_lengths"], t, n)
    assert torch.equal(out["spans"][2], res.spans) and torch.equal(_bits(out["conf"][2]), _bits(res.conf))
    al = state.alignments()
    assert [[x[0] for x in a["ensemble_"]] for a in al] == [h["ensemble_"] for h in hyps]
    got, want = state.read(), plain_state.read()
    assert got["ensemble_wer"] == S.wer_from_counts(c)["wer"]
    assert got["alignment_wer"] == want["alignment_wer"] and got["fuse_coord_wer"] == want["fuse_coord_wer"]
    assert got["wer"] == min(got["alignment_wer"], got["fuse_coord_wer"], got["ensemble_wer"], 200)
    assert got["loss"] == want["loss"]
    # decode_outputs takes the same argument
    lists = S.decode_outputs({k: out[k] for k in ALL + ("input_lengths",)}, 5, ensembles=_spec())
    assert lists["ensemble_"] == [h["ensemble_"] for h in hyps] and lists["fuse_coord_"] == [h["fuse_coord_"] for h in hyps]


@pytest.fixture(scope="module")
def eager(fx, model):
    """The unpadded eager eval_step (T = 26) with the ensemble and alignment, once."""
    import scattennet_amd as S
    dev = _dev()
    state = S.EvalState(model, capacity=3, log_width=13, align=True, ensembles=_spec())
    out = S.eval_step(model, _src(fx, dev), state)
    return {"tokens": out["tokens"].cpu(), "lengths": out["lengths"].cpu(), "counts": out["counts"].cpu(),
            "spans": out["spans"].cpu(), "conf": out["conf"].cpu(), "alignments": state.alignments(2)}


@pytest.mark.parametrize("bucket", [28, 32, 40])
def test_bucketed_eval_step_ensemble_equals_the_unpadded_eager_step(fx, model, eager, bucket):
    """Three feeds: the eager, the capture and the replay path of the bucket."""
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(bucket,), label_bucket=3, capacity=9, align=True,
                             ensembles=_spec())
    for i in range(3):
        out = bes.step(src)
        assert out[ENS].shape == (3, 13, out["left"].shape[-1]) and out["tokens"].shape == (3, 3, 13), (bucket, i)
        for k in ("tokens", "lengths", "counts", "spans"):
            assert torch.equal(out[k].cpu(), eager[k]), (bucket, i, k)  # the plain heads and the ensemble
    assert bes.graphs_captured == 1
    hyps = bes.hypotheses()
    assert len(hyps) == 9 and all("ensemble_" in h for h in hyps)
    assert "ensemble_wer" in bes.read()


# ------------------------------------------------------------------ 5: the label-free path
def _unlabelled(src):
    return {k: src[k] for k in ("keypoints", "mask", "valid_len_in")}


def test_predict_is_forward_without_the_losses(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    with torch.no_grad():
        full = model(src)
        pred = model.predict(_unlabelled(src))  # no label key at all
    assert sorted(pred) == sorted(ALL + ("input_lengths", "finite_flags"))
    for k in ALL:
        assert torch.equal(_bits(pred[k]), _bits(full[k])), k
    assert torch.equal(pred["input_lengths"], full["input_lengths"])
    flags = pred["finite_flags"]
    assert flags.dtype == torch.int32 and flags.shape == (10,) and not flags.any()
    assert torch.equal(flags, full["finite_report"][:10])
    bad = _unlabelled(src)
    bad["keypoints"] = src["keypoints"].clone()
    bad["keypoints"][1, 3, 2, 0] = float("nan")
    with torch.no_grad():
        with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
            model.predict(bad)  # check == "sync"
        model.check = "defer"
        try:
            deferred = model.predict(bad)
        finally:
            model.check = "sync"
        assert int(deferred["finite_flags"][0]) & 1
        model.check = "off"
        try:
            off = model.predict(bad)
        finally:
            model.check = "sync"
        assert not off["finite_flags"].any()


def test_recognize_step_equals_eval_step_with_alignment(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    state = S.EvalState(model, heads=("fuse_coord_gloss_logits", "left"), capacity=3, log_width=13, align=True,
                        ensembles=_spec())
    want = S.eval_step(model, src, state)
    rec = S.recognize_step(model, _unlabelled(src), heads=("fuse_coord_gloss_logits", "left"), ensembles=_spec())
    assert isinstance(rec, S.Recognition) and rec.decoded == ("fuse_coord_gloss_logits", "left", ENS)
    for k in ("tokens", "lengths", "spans"):
        assert torch.equal(rec[k], want[k]), k
    assert torch.equal(_bits(rec["conf"]), _bits(want["conf"]))
    assert torch.equal(_bits(rec["align_scores"]), _bits(want["align_scores"]))
    assert model.check == "sync" and not rec["finite_flags"].any()
    assert rec.read() == state.alignments(frame_scale=2)
    assert rec.read(frame_scale=1) == state.alignments()
    ids = S.recognize_step(model, _unlabelled(src), heads=("fuse_coord_gloss_logits", "left"), ensembles=_spec(),
                           align=False)
    assert "spans" not in ids and ids.read() == state.hypotheses()


def _assert_lists(got, want, where):
    assert len(got) == len(want), where
    for b, (g, w) in enumerate(zip(got, want)):
        assert sorted(g) == sorted(w), (where, b)
        for name in w:
            assert [e[:3] for e in g[name]] == [e[:3] for e in w[name]], (where, b, name)
            assert all(abs(a[3] - e[3]) <= 1e-3 for a, e in zip(g[name], w[name])), (where, b, name)


@pytest.mark.parametrize("bucket", [28, 32, 40])
def test_bucketed_recognizer_returns_the_eval_steps_alignments(fx, model, eager, bucket):
    """Eager, captured and replayed uses of a bucket, then a flagged batch and another B."""
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    rec = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(bucket,), ensembles=_spec())
    for i in range(3):
        out = rec.step(_unlabelled(src))
        assert out["tokens"].shape == (3, 3, 13) and out["spans"].shape == (3, 3, 13, 2), (bucket, i)
        assert out[ENS].shape[:2] == (3, 13) and out["left"].shape[:2] == (3, 13)
        assert torch.equal(out["tokens"].cpu(), eager["tokens"]) and torch.equal(out["spans"].cpu(), eager["spans"])
        _assert_lists(out.read(), eager["alignments"], (bucket, i))
    assert rec.graphs_captured == 1 and rec.eager_fallbacks == 0
    if bucket != 32:
        return
    bad = _unlabelled(src)
    bad["keypoints"] = src["keypoints"].clone()
    bad["keypoints"][2, 5, 1, 1] = float("nan")
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        rec.step(bad).read()  # a replay
    # a batch of another B: the eager step, unpadded
    two = {k: v[:2].contiguous() for k, v in src.items()}
    state = S.EvalState(model, capacity=2, log_width=13, align=True, ensembles=_spec())
    S.eval_step(model, two, state)
    out = rec.step(_unlabelled(two))
    assert rec.eager_fallbacks == 1 and out["tokens"].shape == (3, 2, 13)
    assert out.read() == state.alignments(frame_scale=2)
    _assert_lists(rec.step(_unlabelled(src)).read(), eager["alignments"], "after")  # the graph still replays
