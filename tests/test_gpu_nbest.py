"""N-best CTC decoding, bigram rescoring and MBR selection on the MI355X (scattennet_amd/nbest.py;
csrc/decode.hip: sca_ctc_beam_decode_nbest, sca_nbest_rescore, sca_nbest_mbr, sca_nbest_gather)
against the float64 restatement of tests/nbest_ref.py, bitwise across the 1-best decoder, the
grouped / single-head, eager / captured and reduced-precision forms, and inside the bucketed
evaluation and recognition steps on the reference's fixture.

Tokens, lengths, counts, order, loss and best are compared for equality (the inputs' tie margins
are asserted on the CPU, tests/test_nbest.py); scores, totals, posteriors and risks within
|out - ref| <= 1e-3 max(1, |ref|), the project's bound.  Measured maximum of that ratio over all
parity cases on one MI355X: 1.6e-7 for the uncollapsed scores, 7.0e-6 over the rescored chain (at
C = 1124, where a total is near 300 and one fp32 ulp there is 3e-5)."""
import copy

import numpy as np
import pytest
import torch

from tests import decode_ref as D
from tests import nbest_ref as R
from tests.golden_util import load

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's relative bound
MIN_GAP = 1e-4
SHAPES = list(R.CASES)
IDS = ["B%d_T%d_C%d_W%d_N%d" % s for s in SHAPES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _inputs(shape, dev):
    x = torch.from_numpy(R.case_logits(shape)).to(dev)
    return x, torch.tensor(R.CASES[shape][1])


def _lm(C, dev):
    import scattennet_amd as S
    return S.BigramLM(R.random_lm(C), device=dev)


def _assert_list(nb, b, entries, where):
    """Clip b of a single-head NBest equals the restatement's entries; the rest is padding."""
    tokens, lengths, scores, count = (t.cpu().numpy() for t in nb)
    n = len(entries)
    assert int(count[b]) == n, where
    for e, (h, _) in enumerate(entries):
        assert tokens[b, e, :lengths[b, e]].tolist() == h, (where, e)
        assert not tokens[b, e, lengths[b, e]:].any(), (where, e)
    assert not tokens[b, n:].any() and not lengths[b, n:].any() and np.isneginf(scores[b, n:]).all(), where
    return _err(scores[b, :n], [s for _, s in entries])


# ------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chain_against_the_restatement(shape):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    x, il = _inputs(shape, dev)
    ref = R.case_ref(shape)
    nb = S.ctc_decode_nbest_device(x, il, W, N)
    assert nb.tokens.shape == (B, N, T) and nb.tokens.dtype == torch.int32 and nb.scores.dtype == torch.float32
    total, post, order = S.rescore_nbest_device(nb, _lm(C, dev), R.LM_WEIGHT, R.LENGTH_BONUS, R.POSTERIOR_SCALE)
    best, risk, loss = S.mbr_select_device(nb, post)
    by_total = S.select_device(nb, total, order)
    by_risk = S.select_device(nb, total, best)
    total, post, order, best, risk, loss = (t.cpu().numpy() for t in (total, post, order, best, risk, loss))
    errs = []
    for b, clip in enumerate(ref):
        n = len(clip["entries"])
        errs.append(_assert_list(nb, b, clip["entries"], (shape, b)))
        assert order[b, :n].tolist() == clip["order"] and order[b, n:].tolist() == list(range(n, N)), (shape, b)
        assert loss[b, :n, :n].tolist() == clip["loss"].tolist() and int(best[b]) == clip["best"], (shape, b)
        assert not loss[b, n:].any() and not loss[b, :, n:].any(), (shape, b)
        assert np.isneginf(total[b, n:]).all() and not post[b, n:].any() and np.isposinf(risk[b, n:]).all(), (shape, b)
        errs += [_err(total[b, :n], clip["total"]), _err(post[b, :n], clip["posterior"]), _err(risk[b, :n], clip["risk"])]
        assert abs(float(post[b].sum()) - 1.0) <= TOL
        for (t1, n1, v1), e in ((by_total, clip["order"][0]), (by_risk, clip["best"])):
            h = clip["entries"][e][0]
            assert int(n1[b]) == len(h) and t1[b, :len(h)].tolist() == h and not t1[b, len(h):].any(), (shape, b, e)
            assert float(v1[b]) == float(total[b, e]), (shape, b, e)
    print(f"{IDS[SHAPES.index(shape)]}: max err {max(errs):.3e}")
    assert max(errs) <= TOL, errs


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_uncollapsed_list_and_its_first_entry(shape):
    """collapse_repeats = 0: the beams as they are; entry 0 is bitwise the 1-best decoder's output,
    and without table, weight and bonus rescoring is the identity."""
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    x, il = _inputs(shape, dev)
    nb = S.ctc_decode_nbest_device(x, il, W, N, collapse_repeats=False)
    errs = [_assert_list(nb, b, clip["entries"], (shape, b)) for b, clip in enumerate(R.case_ref(shape, False, False))]
    print(f"{IDS[SHAPES.index(shape)]}: max err {max(errs):.3e}")
    assert max(errs) <= TOL
    t1, n1, s1 = S.ctc_decode_device(x, il, W, collapse_repeats=False)
    assert torch.equal(nb.tokens[:, 0], t1) and torch.equal(nb.lengths[:, 0], n1)
    assert torch.equal(_bits(nb.scores[:, 0]), _bits(s1))
    for src in (nb, S.ctc_decode_nbest_device(x, il, W, N)):
        total, post, order = S.rescore_nbest_device(src, None, 0.0, 0.0, R.POSTERIOR_SCALE)
        assert torch.equal(_bits(total), _bits(src.scores))
        assert torch.equal(order, torch.arange(N, dtype=torch.int32, device=dev).expand(B, N))
        with_table = S.rescore_nbest_device(src, _lm(C, dev), 0.0, 0.0, R.POSTERIOR_SCALE)
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(with_table, (total, post, order)))
    want = [R.rescore(c["entries"], posterior_scale=R.POSTERIOR_SCALE)[1] for c in R.case_ref(shape, False, False)]
    total, post, _ = S.rescore_nbest_device(nb, posterior_scale=R.POSTERIOR_SCALE)
    assert max(_err(post[b, :len(w)].cpu().numpy(), w) for b, w in enumerate(want)) <= TOL


def test_host_lists():
    import scattennet_amd as S
    dev = _dev()
    shape = (4, 12, 6, 8, 3)
    x, il = _inputs(shape, dev)
    lists = S.ctc_decode_nbest(x, 8, il, nbest=3)
    ref = R.case_ref(shape)
    assert [[h for h, _ in clip] for clip in lists] == [[h for h, _ in c["entries"]] for c in ref]
    assert all(abs(s - r) <= TOL * max(1.0, abs(r)) for clip, c in zip(lists, ref)
               for (_, s), (_, r) in zip(clip, c["entries"]))


# ------------------------------------------------------------------ 2: bitwise forms
def _chain(S, xs, il, W, N, lm):
    nb = S.ctc_decode_nbest_heads_device(xs, il, W, N)
    total, post, order = S.rescore_nbest_device(nb, lm, R.LM_WEIGHT, R.LENGTH_BONUS, R.POSTERIOR_SCALE)
    best, risk, loss = S.mbr_select_device(nb, post)
    return list(nb) + [total, post, order, best, risk, loss] + list(S.select_device(nb, total, best))


@pytest.mark.parametrize("shape", [(4, 12, 6, 8, 3), (2, 64, 1124, 5, 5)], ids=["C6", "C1124"])
def test_grouped_rows_are_the_single_head_calls(shape):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    il = torch.tensor(R.CASES[shape][1])
    xs = [torch.from_numpy(np.random.default_rng(40 + g).normal(0.0, 4.0, (B, T, C)).astype(np.float32)).to(dev)
          for g in range(3)]
    for collapse in (True, False):
        grouped = S.ctc_decode_nbest_heads_device(xs, il, W, N, collapse)
        assert grouped.tokens.shape == (3, B, N, T) and grouped.count.shape == (3, B)
        for g, x in enumerate(xs):
            one = S.ctc_decode_nbest_device(x, il, W, N, collapse)
            for a, b in zip(grouped, one):
                assert torch.equal(_bits(a[g]), _bits(b)), (collapse, g)
    # the second pass over the grouped list is the second pass over each head's
    lm = _lm(C, dev)
    out = _chain(S, xs, il, W, N, lm)
    for g, x in enumerate(xs):
        for a, b in zip(out, _chain(S, [x], il, W, N, lm)):
            assert torch.equal(_bits(a[g]), _bits(b[0])), g


def test_captured_chain_replayed_on_refilled_inputs_equals_eager():
    import scattennet_amd as S
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    x, il = _inputs(shape, dev)
    il = il.to(dev).to(torch.int32)
    lm = _lm(C, dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(S, [x], il, W, N, lm)  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _chain(S, [x], il, W, N, lm)
    for seed in (None, 7):  # the captured inputs, then refilled ones
        if seed is not None:
            x.copy_(torch.from_numpy(np.random.default_rng(seed).normal(0.0, 4.0, (B, T, C)).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs, _chain(S, [x], il, W, N, lm))):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_reduced_precision_logits_take_the_fp32_view(dtype):
    import scattennet_amd as S
    dev = _dev()
    shape = (4, 12, 6, 8, 3)
    x, il = _inputs(shape, dev)
    low = x.to(dtype)
    for fn, arg, ref_arg in ((S.ctc_decode_nbest_device, low, low.float()),
                             (S.ctc_decode_nbest_heads_device, [low, low], [low.float(), low.float()])):
        got, want = fn(arg, il, 8, 3), fn(ref_arg, il, 8, 3)
        assert got.scores.dtype == dtype and torch.equal(got.scores, want.scores.to(dtype))
        for a, b in zip((got.tokens, got.lengths, got.count), (want.tokens, want.lengths, want.count)):
            assert torch.equal(a, b)
    total, post, order = S.rescore_nbest_device(got)  # a reduced-precision list is rescored in fp32
    assert total.dtype == torch.float32 and torch.equal(total, got.scores.float())


# ------------------------------------------------------------------ 3: the steps
@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


@pytest.fixture(scope="module")
def model(fx):
    """The fixture model, built as tests/test_gpu_ensemble.py builds it; eval mode, never modified."""
    import scattennet_amd as S
    dev = _dev()
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


def _src(fx, dev):
    return {k: v.to(dev) for k, v in fx["in"].items()}


def _unlabelled(src):
    return {k: src[k] for k in ("keypoints", "mask", "valid_len_in")}


HEADS = ("alignment_gloss_logits", "fuse_coord_gloss_logits")
BUCKET = 32
BEAM = R.MODEL_BEAM  # at this width the fixture's logits keep their tie margins (tests/test_nbest.py)


def _spec(fx, dev):
    import scattennet_amd as S
    return S.Rescoring(nbest=3, lm=_lm(fx["meta"]["vocab"], dev), lm_weight=R.LM_WEIGHT, length_bonus=R.LENGTH_BONUS,
                       posterior_scale=R.POSTERIOR_SCALE, select="mbr")


def _restated(out, fx):
    """The restatement's chain on the step's own logits: per head, per clip."""
    lens = out["input_lengths"].cpu().numpy()
    res = [R.full(out[k].double().cpu().numpy(), lens, BEAM, 3, True, R.random_lm(fx["meta"]["vocab"]), R.LM_WEIGHT,
                  R.LENGTH_BONUS, R.POSTERIOR_SCALE) for k in HEADS]
    for head in res:  # a condition on the inputs, as in tests/test_nbest.py
        for clip in head:
            print({k: "%.2e" % v for k, v in clip["gaps"].items()})
            assert min(clip["gaps"].values()) >= MIN_GAP, clip["gaps"]
    return res


def _assert_selection(out, res, where):
    tokens, lengths = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy()
    picked = []
    for g, head in enumerate(res):
        for b, clip in enumerate(head):
            h = clip["entries"][clip["best"]][0]
            assert tokens[g, b, :lengths[g, b]].tolist() == h and not tokens[g, b, lengths[g, b]:].any(), (where, g, b)
            assert int(out["nbest_count"][g, b]) == len(clip["entries"]), (where, g, b)
            picked.append(h)
    return picked


def test_bucketed_recognizer_with_rescoring(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = _unlabelled(_src(fx, dev))
    absent = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(BUCKET,)).step(src)
    none = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(BUCKET,), rescoring=None).step(src)
    assert sorted(absent) == sorted(none) and not any(k.startswith("nbest") for k in none)
    for k in absent:
        same = torch.equal(_bits(absent[k]), _bits(none[k])) if absent[k].dtype == torch.float32 else \
            torch.equal(absent[k], none[k])
        assert same, k
    assert absent.read() == none.read()
    rec = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(BUCKET,), beam_size=BEAM, rescoring=_spec(fx, dev))
    res = None
    for i in range(3):  # the eager, the capture and the replay path of the bucket
        out = rec.step(src)
        assert out["tokens"].shape == (2, 3, 13) and out["nbest_tokens"].shape == (2, 3, 3, 13), i
        assert out["nbest_totals"].shape == out["nbest_posterior"].shape == out["nbest_lengths"].shape == (2, 3, 3)
        res = res or _restated(out, fx)
        _assert_selection(out, res, i)
        clips = out.read()
        assert len(clips) == 3 and sorted(clips[0]) == ["alignment_", "alignment_nbest", "fuse_coord_", "fuse_coord_nbest"]
        for b, clip in enumerate(clips):
            for g, name in enumerate(("alignment_", "fuse_coord_")):
                want = res[g][b]
                got = clip[name + "nbest"]
                assert [e[0] for e in got] == [want["entries"][e][0] for e in want["order"]], (i, b, name)
                assert _err([e[1] for e in got], want["total"][want["order"]]) <= TOL
                assert _err([e[2] for e in got], want["posterior"][want["order"]]) <= TOL
                # the aligned hypothesis is the selected one
                assert [e[0] for e in clip[name]] == want["entries"][want["best"]][0], (i, b, name)
    assert rec.graphs_captured == 1 and rec.eager_fallbacks == 0


def test_bucketed_eval_step_with_rescoring(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    kw = dict(batch_size=3, frame_buckets=(BUCKET,), label_bucket=3, capacity=9)
    a, b = S.BucketedEvalStep(model, **kw), S.BucketedEvalStep(model, rescoring=None, **kw)
    absent, none = a.step(src), b.step(src)
    assert sorted(absent) == sorted(none) and not any(k.startswith("nbest") for k in none)
    for k in ("tokens", "lengths", "counts", "finite_report") + HEADS:
        assert torch.equal(_bits(absent[k]), _bits(none[k])), k
    assert a.read() == b.read() and a.hypotheses() == b.hypotheses()
    bes = S.BucketedEvalStep(model, beam_size=BEAM, rescoring=_spec(fx, dev), **kw)
    res = None
    for i in range(3):
        out = bes.step(src)
        assert out["tokens"].shape == (2, 3, 13) and out["nbest_tokens"].shape == (2, 3, 3, 13), i
        res = res or _restated(out, fx)
        picked = _assert_selection(out, res, i)
    assert bes.graphs_captured == 1
    labels, lab_len = fx["in"]["gloss_labels"].numpy(), fx["in"]["gloss_lengths"].numpy()
    refs = [labels[b, :lab_len[b]].tolist() for b in range(3)]
    got, raw = bes.read(), bes.state.raw()
    for g, name in enumerate(("alignment_", "fuse_coord_")):
        hyps = picked[3 * g:3 * g + 3]
        assert got[name + "wer"] == D.wer_list(refs, hyps)["wer"], name
        counts = np.array([D.wer_single(r, h) for r, h in zip(refs, hyps)]).sum(0)
        assert raw["totals"][g].tolist() == (3 * counts).tolist(), name
    assert [h["fuse_coord_"] for h in bes.hypotheses()[:3]] == picked[3:]
