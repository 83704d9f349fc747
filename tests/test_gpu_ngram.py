"""The backoff n-gram gloss model on the MI355X (scattennet_amd/ngram.py; csrc/ctc.h:
ctc_ngram_prior; sca_nbest_rescore_ngram, sca_mwer_heads_fwd_ngram) against the float64
restatement of tests/ngram_ref.py, and bitwise against the dense table's kernels, the lm = None
call, the single-head call and the eager call.

Order, loss, best and the selected tokens are compared for equality (the inputs' tie margins and
the look-up outcomes are asserted on the CPU, tests/test_ngram.py); totals, posteriors and risks
within |out - ref| <= 1e-3 max(1, |ref|), the project's bound (DESIGN.md §5c.6 records the
measured maximum)."""
import functools
from unittest import mock

import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import nbest_ref as R
from tests import ngram_ref as NG
from tests.mwer_gpu import _nbest
from tests.test_gpu_nbest import _bits, _dev, _err, _inputs, _src, fx, model  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's relative bound
SHAPES = NG.SHAPES
IDS = ["B%d_T%d_C%d_W%d_N%d" % s for s in SHAPES]
WEIGHTS = (R.LM_WEIGHT, R.LENGTH_BONUS, R.POSTERIOR_SCALE)


@functools.lru_cache(maxsize=None)
def _lm(shape, order=3):
    """The case's model on the device, built once."""
    import scattennet_amd as S
    return NG.build(S.NGramLM, NG.case_model(shape, order), _dev())


@functools.lru_cache(maxsize=None)
def _list(shape):
    """The case's collapsed n-best list, decoded once and never modified."""
    import scattennet_amd as S
    x, il = _inputs(shape, _dev())
    return S.ctc_decode_nbest_device(x, il, shape[3], shape[4])


def _same(got, want, where):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b)), (where, i)


# ------------------------------------------------------------------ 1: order 3 against the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_trigram_chain_against_the_restatement(shape):
    import scattennet_amd as S
    B, T, C, W, N = shape
    nb, lm = _list(shape), _lm(shape)
    assert lm.order == 3 and lm.num_entries[2] > 0
    total, post, order = S.rescore_nbest_device(nb, lm, *WEIGHTS)
    best, risk, loss = S.mbr_select_device(nb, post)
    by_total, by_risk = S.select_device(nb, total, order), S.select_device(nb, total, best)
    total, post, order, best, risk, loss = (t.cpu().numpy() for t in (total, post, order, best, risk, loss))
    tokens, lengths = nb.tokens.cpu().numpy(), nb.lengths.cpu().numpy()
    errs = []
    for b, clip in enumerate(NG.case_ref(shape)[0]):
        n = len(clip["entries"])
        assert int(nb.count[b]) == n, (shape, b)
        for e, (h, _) in enumerate(clip["entries"]):
            assert tokens[b, e, :lengths[b, e]].tolist() == h, (shape, b, e)
        assert order[b, :n].tolist() == clip["order"] and order[b, n:].tolist() == list(range(n, N)), (shape, b)
        assert loss[b, :n, :n].tolist() == clip["loss"].tolist() and int(best[b]) == clip["best"], (shape, b)
        assert np.isneginf(total[b, n:]).all() and not post[b, n:].any(), (shape, b)
        errs += [_err(total[b, :n], clip["total"]), _err(post[b, :n], clip["posterior"]), _err(risk[b, :n], clip["risk"])]
        for (t1, n1, v1), e in ((by_total, clip["order"][0]), (by_risk, clip["best"])):
            h = clip["entries"][e][0]
            assert int(n1[b]) == len(h) and t1[b, :len(h)].tolist() == h and not t1[b, len(h):].any(), (shape, b, e)
            assert float(v1[b]) == float(total[b, e]), (shape, b, e)
    print(f"{IDS[SHAPES.index(shape)]}: max err {max(errs):.3e}")
    assert max(errs) <= TOL, errs


# ------------------------------------------------------------------ 2, 3: bitwise against the dense kernels
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_sparse_orders_1_and_2_are_bitwise_the_dense_call(shape, order):
    import scattennet_amd as S
    nb, lm = _list(shape), _lm(shape, order)
    assert lm.order == order and (order == 1 or 0 < lm.num_entries[1] < shape[2] ** 2)
    dense = lm.to_bigram()
    assert dense.table.device == nb.tokens.device
    _same(S.rescore_nbest_device(nb, lm, *WEIGHTS), S.rescore_nbest_device(nb, dense, *WEIGHTS), (shape, order))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weight_and_bonus_0_are_bitwise_the_call_without_a_model(shape):
    import scattennet_amd as S
    nb = _list(shape)
    want = S.rescore_nbest_device(nb, None, 0.0, 0.0, R.POSTERIOR_SCALE)
    for order in (1, 2, 3):
        _same(S.rescore_nbest_device(nb, _lm(shape, order), 0.0, 0.0, R.POSTERIOR_SCALE), want, (shape, order))


# ------------------------------------------------------------------ 4: grouped and captured forms
def _chain(S, xs, il, W, N, lm):
    nb = S.ctc_decode_nbest_heads_device(xs, il, W, N)
    total, post, order = S.rescore_nbest_device(nb, lm, *WEIGHTS)
    best, risk, loss = S.mbr_select_device(nb, post)
    return list(nb) + [total, post, order, best, risk, loss] + list(S.select_device(nb, total, best))


def test_grouped_rows_are_the_single_head_calls():
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 20, 33, 32, 32)
    B, T, C, W, N = shape
    il = torch.tensor(R.CASES[shape][1])
    xs = [torch.from_numpy(np.random.default_rng(40 + g).normal(0.0, 4.0, (B, T, C)).astype(np.float32)).to(dev)
          for g in range(2)]
    lm = _lm(shape)
    out = _chain(S, xs, il, W, N, lm)
    assert out[4].shape == (2, B, N)
    for g, x in enumerate(xs):
        for i, (a, b) in enumerate(zip(out, _chain(S, [x], il, W, N, lm))):
            assert torch.equal(_bits(a[g]), _bits(b[0])), (g, i)


def test_captured_chain_replayed_on_refilled_inputs_equals_eager():
    import scattennet_amd as S
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    x, il = _inputs(shape, dev)
    il = il.to(dev).to(torch.int32)
    lm = _lm(shape)
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


# ------------------------------------------------------------------ 5: the MWER prior
MWER_SHAPES = [(5, 16, 4, 8, 8), (3, 20, 33, 32, 32)]  # the two smallest


def _mwer(shape, lm, **kw):
    """`mwer_loss` with the reference slot on the case's uncollapsed lists: (loss, details, dlogits)."""
    import scattennet_amd as S
    dev = _dev()
    logits, in_len, lists, refs = M.case_inputs_ext(shape)
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    ref, ref_len = M.pack_refs(refs)
    loss, det = S.mwer_loss(x, torch.tensor(in_len), torch.from_numpy(ref), torch.from_numpy(ref_len),
                            nbest=_nbest(lists, shape[4], shape[1], dev), posterior_scale=M.POSTERIOR_SCALE,
                            return_details=True, reference=True, lm=lm, lm_weight=M.LM_WEIGHT,
                            length_bonus=M.LENGTH_BONUS, **kw)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), det, x.grad


@pytest.mark.parametrize("shape", MWER_SHAPES, ids=IDS[:2])
def test_mwer_with_the_trigram_prior_against_the_restatement(shape):
    logits, in_len, lists, refs = M.case_inputs_ext(shape)
    table = NG.case_model(shape)
    with mock.patch.object(M, "prior", lambda h, lm, lw, lb: NG.prior(table, h, lw, lb)):  # the restatement's prior
        want = M.mwer(logits, in_len, lists, refs, M.POSTERIOR_SCALE, n_max=shape[4], with_ref=True, lm=None,
                      lm_weight=M.LM_WEIGHT, length_bonus=M.LENGTH_BONUS)
    loss, det, dx = _mwer(shape, _lm(shape))
    figs = {"loss": _err(loss.cpu(), want["loss"]), "posterior": _err(det["posterior"].cpu(), want["posterior"]),
            "risk": _err(det["risk"].cpu(), want["risk"]), "dlogits": _err(dx.cpu(), want["dlogits"])}
    print(shape, {k: f"{v:.3g}" for k, v in figs.items()})
    assert np.array_equal(det["errors"].cpu().numpy().astype(np.int64), want["errors"])
    assert np.array_equal(det["ref_valid"].cpu().numpy().astype(np.int64), want["ref_valid"])
    assert max(figs.values()) <= TOL, figs


@pytest.mark.parametrize("shape", MWER_SHAPES, ids=IDS[:2])
def test_mwer_with_an_order_2_model_is_bitwise_the_dense_prior(shape):
    lm = _lm(shape, 2)
    (la, da, ga), (lb, db, gb) = _mwer(shape, lm), _mwer(shape, lm.to_bigram())
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb))
    assert sorted(da) == sorted(db)
    for k in da:
        assert torch.equal(_bits(da[k]), _bits(db[k])), k


def test_the_c_entry_points_reject_a_bad_model():
    """Validated before any GPU call: ValueError from the C ABI for a struct the class would never build."""
    import ctypes

    import scattennet_amd as S
    from scattennet_amd import _lib as L
    shape = (5, 16, 4, 8, 8)
    nb, lm = _list(shape), _lm(shape)
    total, post, order = (torch.empty_like(nb.scores), torch.empty_like(nb.scores), torch.empty_like(nb.lengths))
    for field, value in (("order", 0), ("order", 4), ("C", 0), ("C", 8193), ("n_bi", -1), ("n_tri", -1),
                         ("uni_lp", None), ("bi_ptr", None), ("tri_ptr", None), ("tri_tok", None)):
        s = L.NgramLm.from_buffer_copy(lm.struct)
        setattr(s, field, value)
        with pytest.raises(ValueError, match="sca_nbest_rescore_ngram"):
            L.check(L.lib().sca_nbest_rescore_ngram(L.ptr(nb.tokens), L.ptr(nb.lengths), L.ptr(nb.scores),
                                                    L.ptr(nb.count), 1, shape[0], shape[4], shape[1], ctypes.byref(s),
                                                    0.5, 0.0, 1.0, L.ptr(total), L.ptr(post), L.ptr(order),
                                                    L.stream_handle()), "sca_nbest_rescore_ngram")
    with pytest.raises(ValueError, match="classes"):
        S.mwer_loss(torch.zeros(2, 6, 5, device=_dev()), torch.tensor([6, 6]), torch.tensor([[1], [2]]),
                    torch.tensor([1, 1]), lm=lm, lm_weight=0.5)


# ------------------------------------------------------------------ 6: the bucketed step
HEADS = ("alignment_gloss_logits", "fuse_coord_gloss_logits")


def test_bucketed_eval_step_with_a_trigram_equals_the_unbucketed_decode(fx, model):  # noqa: F811
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    C = fx["meta"]["vocab"]
    lm = NG.build(S.NGramLM, NG.random_ngram(C, 3, 11), dev)
    spec = S.Rescoring(3, lm, lm_weight=R.LM_WEIGHT, length_bonus=R.LENGTH_BONUS, posterior_scale=R.POSTERIOR_SCALE,
                       select="mbr")
    bes = S.BucketedEvalStep(model, beam_size=R.MODEL_BEAM, rescoring=spec, batch_size=3, frame_buckets=(32,),
                             label_bucket=3, capacity=9)
    for i in range(3):  # the eager, the capture and the replay path of the bucket
        out = bes.step(src)
        want = S.rescored_decode([out[k] for k in HEADS], out["input_lengths"], R.MODEL_BEAM, spec)
        assert out["tokens"].shape == want["tokens"].shape == (2, 3, 13), i
        for k in ("tokens", "lengths", "nbest_tokens", "nbest_lengths", "nbest_totals", "nbest_posterior",
                  "nbest_order", "nbest_count", "nbest_risk", "nbest_best"):
            assert torch.equal(_bits(out[k]), _bits(want[k])), (i, k)
    assert bes.graphs_captured == 1
    # the model changes the selection's totals: the same step without it differs
    plain = S.rescored_decode([out[k] for k in HEADS], out["input_lengths"], R.MODEL_BEAM,
                              S.Rescoring(3, None, length_bonus=R.LENGTH_BONUS, posterior_scale=R.POSTERIOR_SCALE,
                                          select="mbr"))
    assert not torch.equal(plain["nbest_totals"], out["nbest_totals"])
