"""Shallow fusion on the MI355X (csrc/decode.hip: sca_ctc_beam_decode_fused_nbest and its grouped
form; scattennet_amd/nbest.py) against the float64 restatement of tests/fusion_ref.py, bitwise
against the unfused n-best decode at weight 0 and bonus 0, across the grouped / single-head and
eager / captured forms, through `rescored_decode` and inside the evaluation and recognition steps.

Tokens, lengths, counts, order and best are compared for equality (the inputs' tie margins and
their float32 stability are asserted on the CPU, tests/test_fusion.py); scores and totals within
|out - ref| <= 1e-3 max(1, |ref|), the project's bound.  Measured maxima on one MI355X are in
DESIGN.md §5c.5."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import fusion_ref as F
from tests import nbest_ref as R
from tests.golden_util import load

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's relative bound
MIN_GAP = 1e-4
SHAPES = list(F.CASES)
IDS = ["B%d_T%d_C%d_W%d_N%d" % s for s in SHAPES]
ERR_ARG = 1


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()) if ref.size else 0.0


def _lm(table, dev):
    import scattennet_amd as S
    return S.BigramLM(np.asarray(table, np.float32), device=dev)


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
@pytest.mark.parametrize("w", F.WEIGHTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_list_against_the_restatement(shape, w):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    x = torch.from_numpy(F.case_logits(shape)).to(dev)
    il = torch.tensor(F.CASES[shape][1])
    lm = _lm(R.random_lm(C), dev)
    errs = []
    for collapse in (True, False):
        ref = F.case_ref(shape, w, collapse)
        nb = S.ctc_decode_fused_nbest_device(x, il, W, lm, w, F.BONUS, N, collapse)
        assert nb.tokens.shape == (B, N, T) and nb.tokens.dtype == torch.int32 and nb.scores.dtype == torch.float32
        total, _, order = S.rescore_nbest_device(nb, lm, w, F.BONUS, F.POSTERIOR_SCALE)
        total, order = total.cpu().numpy(), order.cpu().numpy()
        for b, clip in enumerate(ref):
            n = len(clip["entries"])
            errs.append(_assert_list(nb, b, clip["entries"], (shape, w, collapse, b)))
            assert order[b, :n].tolist() == clip["order"], (shape, w, collapse, b)
            errs.append(_err(total[b, :n], clip["total"]))
            if not collapse:  # the rescorer turns the scores into the keys the search ranked by
                errs.append(_err(total[b, :n], clip["keys"]))
                assert clip["order"] == list(range(n))
    print(f"{IDS[SHAPES.index(shape)]} w={w}: max err {max(errs):.3e}")
    assert max(errs) <= TOL, errs


def _one_clip(case, N, collapse=False):
    x, lm, w, bonus, W = case
    return x, lm, w, bonus, W, F.fused_nbest(x[0], x.shape[1], W, N, collapse, lm, w, bonus, "per_beam")


def test_constructed_preselection_case():
    """The label outside the frame's top-(W + 1) by lp enters the beam through its bigram."""
    import scattennet_amd as S
    dev = _dev()
    x, lm, w, W = F.constructed_case()
    x, lm, w, bonus, W, (entries, _, _) = _one_clip((x, lm, w, 0.0, W), W)
    nb = S.ctc_decode_fused_nbest_device(torch.from_numpy(x).to(dev), [3], W, _lm(lm, dev), w, bonus, W, False)
    assert [list(h) for h, _ in entries] == [[1], [1, 9]]
    assert _assert_list(nb, 0, entries, "constructed") <= TOL


def test_fusion_wins_case():
    import scattennet_amd as S
    dev = _dev()
    x, lm, w, bonus, W, (entries, keys, _) = _one_clip(F.wins_case(), 3)
    xd, table = torch.from_numpy(x).to(dev), _lm(lm, dev)
    il = [x.shape[1]]
    fused = S.ctc_decode_fused_nbest_device(xd, il, W, table, w, bonus, W, False)
    assert _assert_list(fused, 0, entries, "wins") <= TOL
    best_fused = S.rescore_nbest_device(fused, table, w, bonus)[0].max().item()
    best_unfused = S.rescore_nbest_device(S.ctc_decode_nbest_device(xd, il, W, W, False), table, w, bonus)[0].max().item()
    assert abs(best_fused - max(keys)) <= TOL * abs(max(keys))
    assert best_fused - best_unfused > 1.0, (best_fused, best_unfused)  # tests/test_fusion.py: WINS_MARGIN


def test_list_overflow_takes_the_round_by_round_selection():
    import scattennet_amd as S
    dev = _dev()
    x, lm, w, bonus = F.fallback_case()
    _, T, C, W, N = F.FALLBACK_SHAPE
    entries, _, _ = F.fused_nbest(x[0], T, W, N, False, lm, w, bonus, "per_beam")
    nb = S.ctc_decode_fused_nbest_device(torch.from_numpy(x).to(dev), [T], W, _lm(lm, dev), w, bonus, N, False)
    assert _assert_list(nb, 0, entries, "fallback") <= TOL


def test_length_bonus_alone_and_host_lists():
    import scattennet_amd as S
    dev = _dev()
    shape = (4, 12, 6, 8, 3)
    x = torch.from_numpy(F.case_logits(shape)).to(dev)
    il = F.CASES[shape][1]
    lists = S.ctc_decode_fused_nbest(x, 8, il, None, 0.0, 0.7, nbest=3)
    for b, clip in enumerate(lists):
        entries, _, gaps = F.fused_nbest(F.case_logits(shape)[b], il[b], 8, 3, True, None, 0.0, 0.7, "per_beam")
        assert min(gaps.values()) > MIN_GAP
        assert [h for h, _ in clip] == [h for h, _ in entries], b
        assert _err([s for _, s in clip], [s for _, s in entries]) <= TOL


# ------------------------------------------------------------------ 2: bitwise forms
@pytest.mark.parametrize("shape", [(5, 16, 4, 8, 8), (2, 64, 1124, 5, 5)], ids=["C4", "C1124"])
def test_weight_zero_is_bitwise_the_unfused_decode(shape):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    il = torch.tensor(F.CASES[shape][1])
    xs = [torch.from_numpy(np.random.default_rng(40 + g).normal(0.0, 4.0, (B, T, C)).astype(np.float32)).to(dev)
          for g in range(3)]
    lm = _lm(R.random_lm(C), dev)
    for collapse in (True, False):
        for table in (None, lm):
            want = S.ctc_decode_nbest_heads_device(xs, il, W, N, collapse)
            got = S.ctc_decode_fused_nbest_heads_device(xs, il, W, table, 0.0, 0.0, N, collapse)
            for a, b in zip(got, want):
                assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (collapse, table)
            want = S.ctc_decode_nbest_device(xs[0], il, W, N, collapse)
            got = S.ctc_decode_fused_nbest_device(xs[0], il, W, table, 0.0, 0.0, N, collapse)
            for a, b in zip(got, want):
                assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (collapse, table)


@pytest.mark.parametrize("shape", [(4, 12, 6, 8, 3), (2, 64, 1124, 5, 5)], ids=["C6", "C1124"])
def test_grouped_rows_are_the_single_head_calls(shape):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    il = torch.tensor(F.CASES[shape][1])
    xs = [torch.from_numpy(np.random.default_rng(40 + g).normal(0.0, 4.0, (B, T, C)).astype(np.float32)).to(dev)
          for g in range(3)]
    lm = _lm(R.random_lm(C), dev)
    for collapse in (True, False):
        grouped = S.ctc_decode_fused_nbest_heads_device(xs, il, W, lm, 0.5, F.BONUS, N, collapse)
        assert grouped.tokens.shape == (3, B, N, T) and grouped.count.shape == (3, B)
        for g, x in enumerate(xs):
            one = S.ctc_decode_fused_nbest_device(x, il, W, lm, 0.5, F.BONUS, N, collapse)
            for a, b in zip(grouped, one):
                assert torch.equal(_bits(a[g]), _bits(b)), (collapse, g)


def test_captured_decode_replayed_on_refilled_inputs_equals_eager():
    import scattennet_amd as S
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    x = torch.from_numpy(F.case_logits(shape)).to(dev)
    il = torch.tensor(F.CASES[shape][1]).to(dev).to(torch.int32)
    lm = _lm(R.random_lm(C), dev)

    def run():
        return list(S.ctc_decode_fused_nbest_heads_device([x], il, W, lm, 3.0, F.BONUS, N))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    for seed in (None, 7):  # the captured inputs, then refilled ones
        if seed is not None:
            x.copy_(torch.from_numpy(np.random.default_rng(seed).normal(0.0, 4.0, (B, T, C)).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs, run())):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)


# ------------------------------------------------------------------ 3: the chain
def test_rescored_decode_with_fusion_is_the_restated_chain():
    import scattennet_amd as S
    dev = _dev()
    shape, w = (4, 12, 6, 8, 3), 0.5
    B, T, C, W, N = shape
    x = torch.from_numpy(F.case_logits(shape)).to(dev)
    il = torch.tensor(F.CASES[shape][1])
    lm = _lm(R.random_lm(C), dev)
    spec = S.Rescoring(N, lm, w, F.BONUS, F.POSTERIOR_SCALE, select="mbr", fusion=True)
    out = S.rescored_decode([x], il, W, spec)
    ref = F.case_ref(shape, w)
    tokens, lengths = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy()
    totals, order = out["nbest_totals"].cpu().numpy(), out["nbest_order"].cpu().numpy()
    for b, clip in enumerate(ref):
        n, h = len(clip["entries"]), clip["entries"][clip["best"]][0]
        assert int(out["nbest_count"][0, b]) == n and int(out["nbest_best"][0, b]) == clip["best"], b
        assert tokens[0, b, :lengths[0, b]].tolist() == h and not tokens[0, b, lengths[0, b]:].any(), b
        assert order[0, b, :n].tolist() == clip["order"], b
        assert _err(totals[0, b, :n], clip["total"]) <= TOL
        assert _err(out["nbest_risk"][0, b, :n].cpu().numpy(), clip["risk"]) <= TOL
    unfused = S.rescored_decode([x], il, W, S.Rescoring(N, lm, w, F.BONUS, F.POSTERIOR_SCALE, select="mbr"))
    nb = S.ctc_decode_nbest_heads_device([x], il, W, N)
    assert torch.equal(unfused["nbest_tokens"], nb.tokens) and torch.equal(unfused["nbest_count"], nb.count)


# ------------------------------------------------------------------ 4: the steps
@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


@pytest.fixture(scope="module")
def model(fx):
    """The fixture model, built as tests/test_gpu_nbest.py builds it; eval mode, never modified."""
    import scattennet_amd as S
    dev = _dev()
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


HEADS = ("alignment_gloss_logits", "fuse_coord_gloss_logits")
BUCKET = 32
BEAM = R.MODEL_BEAM
STEP_N, STEP_W, STEP_BONUS = 5, 0.5, 0.2


def _spec(fx, dev, fusion):
    import scattennet_amd as S
    return S.Rescoring(STEP_N, _lm(R.random_lm(fx["meta"]["vocab"]), dev), STEP_W, STEP_BONUS, select="mbr",
                       fusion=fusion)


def _restated(out, fx):
    lens = out["input_lengths"].cpu().numpy()
    res = [F.full(out[k].double().cpu().numpy(), lens, BEAM, STEP_N, True, R.random_lm(fx["meta"]["vocab"]), STEP_W,
                  STEP_BONUS) for k in HEADS]
    for head in res:  # a condition on the inputs, as in tests/test_fusion.py
        for clip in head:
            print({k: "%.2e" % v for k, v in clip["gaps"].items()})
            assert min(clip["gaps"].values()) >= MIN_GAP, clip["gaps"]
    return res


def _assert_steps(step, fx, dev):
    """Three calls of a bucketed step (eager, capture, replay): the selection is the restated
    chain's, and the captured outputs are bitwise the eager ones."""
    first, res = None, None
    for i in range(3):
        out = step()
        res = res or _restated(out, fx)
        tokens, lengths = out["tokens"].cpu().numpy(), out["lengths"].cpu().numpy()
        for g, head in enumerate(res):
            for b, clip in enumerate(head):
                h = clip["entries"][clip["best"]][0]
                assert tokens[g, b, :lengths[g, b]].tolist() == h and not tokens[g, b, lengths[g, b]:].any(), (i, g, b)
                assert int(out["nbest_count"][g, b]) == len(clip["entries"]), (i, g, b)
        keys = [k for k in out if k.startswith("nbest_")] + ["tokens", "lengths"]
        if first is None:
            first = {k: out[k].clone() for k in keys}
        for k in keys:
            assert torch.equal(_bits(first[k]), _bits(out[k])), (i, k)
    return out


def _unfused_is_todays_calls(out, fx, dev):
    """fusion=False: the list is bitwise the unfused grouped decode of the step's own logits."""
    import scattennet_amd as S
    nb = S.ctc_decode_nbest_heads_device([out[k] for k in HEADS], out["input_lengths"], BEAM, STEP_N)
    assert torch.equal(out["nbest_tokens"], nb.tokens) and torch.equal(out["nbest_lengths"], nb.lengths)
    assert torch.equal(out["nbest_count"], nb.count)
    total, _, _ = S.rescore_nbest_device(nb, _lm(R.random_lm(fx["meta"]["vocab"]), dev), STEP_W, STEP_BONUS)
    assert torch.equal(_bits(out["nbest_totals"]), _bits(total))


def test_bucketed_recognizer_with_fusion(fx, model, monkeypatch):
    import scattennet_amd as S
    dev = _dev()
    src = {k: fx["in"][k].to(dev) for k in ("keypoints", "mask", "valid_len_in")}
    rec = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(BUCKET,), beam_size=BEAM,
                               rescoring=_spec(fx, dev, True))
    out = _assert_steps(lambda: rec.step(src), fx, dev)
    assert rec.graphs_captured == 1 and rec.eager_fallbacks == 0
    reads, cpu = [], torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (reads.append(1), cpu(t, *a, **k))[1])
    clips = out.read()
    monkeypatch.undo()
    assert len(reads) == 1 and len(clips) == 3 and "fuse_coord_nbest" in clips[0]
    eager = S.recognize_step(model, src, beam_size=BEAM, rescoring=_spec(fx, dev, True))
    assert [c["fuse_coord_nbest"][0][0] for c in eager.read()] == [c["fuse_coord_nbest"][0][0] for c in clips]
    plain = S.BucketedRecognizer(model, batch_size=3, frame_buckets=(BUCKET,), beam_size=BEAM,
                                 rescoring=_spec(fx, dev, False))
    _unfused_is_todays_calls(plain.step(src), fx, dev)


def test_bucketed_eval_step_with_fusion(fx, model):
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    kw = dict(batch_size=3, frame_buckets=(BUCKET,), label_bucket=3, capacity=9)
    bes = S.BucketedEvalStep(model, beam_size=BEAM, rescoring=_spec(fx, dev, True), **kw)
    _assert_steps(lambda: bes.step(src), fx, dev)
    assert bes.graphs_captured == 1 and bes.state.raw()["steps"] == 3
    eager = S.eval_step(model, src, S.EvalState(model), beam_size=BEAM, rescoring=_spec(fx, dev, True))
    assert eager["nbest_tokens"].shape[:3] == (2, 3, STEP_N)
    plain = S.BucketedEvalStep(model, beam_size=BEAM, rescoring=_spec(fx, dev, False), **kw)
    _unfused_is_todays_calls(plain.step(src), fx, dev)


# ------------------------------------------------------------------ 5: the C ABI
def test_c_abi_rejects_bad_arguments_before_any_gpu_call():
    from scattennet_amd import _lib as L
    _dev()
    lib = L.lib()
    assert lib.sca_ctc_fused_workspace_bytes(2, 3, 16, 33, 8) == lib.sca_ctc_decode_heads_workspace_bytes(2, 3, 16, 33, 8)
    for bad in ((0, 3, 16, 33, 8), (9, 3, 16, 33, 8), (1, 0, 16, 33, 8), (1, 3, 0, 33, 8), (1, 3, 16, 8193, 8),
                (1, 3, 16, 33, 0), (1, 3, 16, 33, 33)):
        assert lib.sca_ctc_fused_workspace_bytes(*bad) == 0, bad
    one = ctypes.c_void_p(8)  # never dereferenced: every call below fails validation
    hx = L.DecodeHeads()
    hx.logits[0] = 8

    def single(B=2, T=4, C=5, W=3, N=3, lw=0.5, lb=0.0, ws=one, x=one):
        return lib.sca_ctc_beam_decode_fused_nbest(x, one, B, T, C, W, N, 1, None, lw, lb, one, one, one, one, ws, None)

    def grouped(G=1, W=3, N=3, ws=one):
        return lib.sca_ctc_beam_decode_heads_fused_nbest(ctypes.byref(hx), G, one, 2, 4, 5, W, N, 1, None, 0.5, 0.0,
                                                         one, one, one, one, ws, None)
    for kw in (dict(B=0), dict(T=0), dict(C=0), dict(C=8193), dict(W=0), dict(W=33, N=33), dict(N=4), dict(N=0),
               dict(ws=None), dict(x=None), dict(lw=float("nan")), dict(lb=float("inf"))):
        assert single(**kw) == ERR_ARG, kw
        assert b"sca_ctc_beam_decode_fused_nbest" in lib.sca_last_error()
    for kw in (dict(G=0), dict(G=9), dict(G=2), dict(N=4), dict(W=33, N=33), dict(ws=None)):
        assert grouped(**kw) == ERR_ARG, kw
