"""GPU parity of the extended MWER loss (the reference as one more entry of the list, the gloss
model's prior inside the posterior, several heads per call) against the float64 restatement of
tests/mwer_ref.py, under the project's bound of 1e-3 (golden_util.rel_err); integers are compared
as integers.  The helpers are tests/mwer_gpu.py's and the kernels on the four n-best cases in
every mode tests/test_gpu_mwer.py's; here are the reference slot's likelihood against the CTC
loss, a hand-built case, the bitwise conditions of the header, the grid form of the per-clip
kernel, and the training steps on tests/golden/model_small.  Every test prints the figures it asserts."""
import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import nbest_ref as NR
from tests.golden_util import close, rel_err
from tests.mwer_gpu import fx  # noqa: F401  (the fixture, by name)
from tests.mwer_gpu import (IDS, SHAPES, TOL, _assert_parity, _bits, _build, _case_run, _dev, _grads, _lm, _run,
                            _same, _trainer)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1: the reference slot
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reference_slot_likelihood_is_the_ctc_loss(shape):
    """loglik[.., N] = -nll of CTCLossOp on the same logits and references, for the clips where
    in_len >= len + repeats (there the loss's rule T_b = max(in_len, 1, S_b) changes nothing)."""
    from scattennet_amd.heads import CTCLossOp
    dev = _dev()
    B, T, C, W, N = shape
    logits, in_len, _, refs = M.case_inputs_ext(shape)
    _, det, _ = _case_run(shape, "reference")
    ref, ref_len = (torch.from_numpy(a).to(dev) for a in M.pack_refs(refs))
    _, nll = CTCLossOp.apply(torch.from_numpy(logits).to(dev), ref, torch.tensor(in_len, dtype=torch.int32, device=dev),
                               ref_len)
    fit = [b for b in range(B) if M.fits(refs[b], in_len[b])]
    assert fit and all(np.isneginf(float(det["loglik"][b, N])) for b in range(B) if b not in fit)
    err = rel_err(det["loglik"][fit, N], -nll.cpu()[fit])
    print(IDS[SHAPES.index(shape)], "clips", fit, "loglik[N] against -nll", err)
    assert err < TOL


# ------------------------------------------------------------------ 2: the hand-built case
def _hand_case():
    """T = 16, H = 4, R = 7, C = 6, N = 4, fill -7 behind count and behind every length.
    0: a reference longer than H with an adjacent repeat ((1, 2, 2, 3, 4, 5, 1): 8 frames of 16)
    1: a reference that does not fit ((1, 1, 2, 2) needs 6 frames of 5)
    2: a duplicate (entry 0 is the reference)
    3: an empty reference, no empty entry: the slot is valid
    4: an empty reference with the empty entry in the list: a duplicate
    5: in_len = 0 (the reference (1) does not fit, the empty entry has likelihood 1)
    6: count = 0 with a fitting reference: a single valid slot, the rows are bitwise 0
    7: equal error counts (2, 2, 2): no gradient without the slot, one with it."""
    x = np.random.default_rng(17).normal(0.0, 1.5, (8, 16, 6)).astype(np.float32)
    lists = [[[1, 2], [3], [1, 2, 3, 4]], [[1], [2, 1]], [[2, 3], [2], [3, 3]], [[1], [2, 4]], [[1], []], [[]], [],
             [[1], [2], [3]]]
    refs = [[1, 2, 2, 3, 4, 5, 1], [1, 1, 2, 2], [2, 3], [], [], [1], [1, 2, 3], [1, 2, 3]]
    return x, [16, 5, 10, 8, 8, 0, 12, 9], lists, refs


def test_hand_built_case():
    dev = _dev()
    x, in_len, lists, refs = _hand_case()
    lm = NR.random_lm(6, seed=3)
    for name, kw in (("acoustic", {}), ("table", dict(lm=lm, lm_weight=M.LM_WEIGHT, length_bonus=M.LENGTH_BONUS))):
        want = M.mwer(x, in_len, lists, refs, 1.0, n_max=4, with_ref=True, **kw)
        assert want["ref_valid"].tolist() == [1, 0, 0, 1, 0, 0, 1, 1]
        assert np.isneginf(want["loglik"][[1, 5], 4]).all() and np.isfinite(want["loglik"][[0, 2, 3, 4, 6, 7], 4]).all()
        assert set(want["errors"][7, :3]) == {2} and np.abs(want["dlogits"][7]).max() >= 1e-3
        assert not M.mwer(x[7:], in_len[7:], lists[7:], refs[7:])["dlogits"].any()  # without the slot: none
        loss, det, dx = _run(x, in_len, lists, refs, 4, 4, dev, 1.0, fill=-7, reference=True, **kw)
        _assert_parity("hand-built " + name, loss, det, dx, want)
        assert float(det["loglik"][2, 4]) == float(det["loglik"][2, 0])  # the duplicate: same labels, same lattice
        assert float(det["posterior"][6, 4]) == 1.0 and not _bits(dx[6]).any() and not _bits(dx[5]).any()
        assert float(det["risk"][6]) == 0.0 and dx[7].abs().max() > 1e-3 and dx[0].abs().max() > 0
        assert not det["errors"][:, 4].any() and float(det["loglik"][5, 0]) == 0.0
        for b in range(8):
            assert not dx[b, in_len[b]:].any() and not det["posterior"][b, len(lists[b]):4].any()


# ------------------------------------------------------------------ 3: the bitwise conditions
def test_weight_zero_and_bonus_zero_with_a_table_is_the_call_without_one():
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    logits, in_len, lists, refs = M.case_inputs_ext(shape)
    base = _case_run(shape, "reference")
    zero = _run(logits, in_len, lists, refs, shape[4], shape[1], dev, M.POSTERIOR_SCALE, reference=True,
                lm=M.random_lm(shape[2]), lm_weight=0.0, length_bonus=0.0)
    _same(zero, base, "weight 0")
    assert base[2].abs().max() > 0


def test_head_of_a_grouped_call_is_the_single_head_call():
    """G = 3: the logits of case (5, 16, 4, 8, 8) under three seeds, each head with its own list
    (the restatement's for seed 0, shifted for the others), the reference and the table on."""
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    _, in_len, lists, refs = M.case_inputs_ext(shape)
    xs = tuple(np.random.default_rng(s).normal(0.0, 4.0, (B, T, C)).astype(np.float32) for s in (0, 1, 2))
    heads_lists = (lists, lists[1:] + lists[:1], [l[::-1] for l in lists])  # entries that do not fit are fine
    kw = dict(reference=True, lm=M.random_lm(C), lm_weight=M.LM_WEIGHT, length_bonus=M.LENGTH_BONUS)
    loss, det, dxs = _run(xs, in_len, heads_lists, refs, N, T, dev, M.POSTERIOR_SCALE, **kw)
    assert loss.shape == (3,) and det["loglik"].shape == (3, B, N + 1) and det["ref_valid"].shape == (3, B)
    for g in range(3):
        one = _run(xs[g], in_len, heads_lists[g], refs, N, T, dev, M.POSTERIOR_SCALE, **kw)
        _same((loss[g], {k: v[g] for k, v in det.items()}, dxs[g]), one, f"head {g}")
        assert dxs[g].abs().max() > 0
    assert not torch.equal(dxs[0], dxs[1])


def test_captured_forward_and_backward_replay_bitwise():
    import scattennet_amd as S
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    logits, in_len, _, refs = M.case_inputs_ext(shape)
    xs = [torch.from_numpy(logits).to(dev).requires_grad_(True), torch.from_numpy(logits[::-1].copy()).to(dev).requires_grad_(True)]
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    ref, ref_len = (torch.from_numpy(a).to(dev) for a in M.pack_refs(refs))
    lm = _lm(M.random_lm(C), dev)

    def chain():
        for x in xs:
            x.grad = None
        loss, det = S.mwer_loss(xs, il, ref, ref_len, beam_size=W, nbest_size=N, posterior_scale=M.POSTERIOR_SCALE,
                                return_details=True, reference=True, lm=lm, lm_weight=M.LM_WEIGHT,
                                length_bonus=M.LENGTH_BONUS, fusion=True)
        loss.sum().backward()
        return [loss.detach(), det["loglik"], det["posterior"], det["errors"], det["ref_valid"], det["risk"],
                xs[0].grad, xs[1].grad]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for seed in (None, 7):  # the captured inputs, then refilled ones
        if seed is not None:
            with torch.no_grad():
                for i, x in enumerate(xs):
                    x.copy_(torch.from_numpy(np.random.default_rng(seed + i).normal(0.0, 4.0, (B, T, C)).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)
        assert got[6].abs().max() > 0 and got[7].abs().max() > 0 and got[4].any()


# ------------------------------------------------------------------ 4: the grid form
def test_many_pairs_take_the_grid_form_of_the_per_clip_kernel():
    """G B = 70 > 64 (G = 2, B = 35): four pairs per workgroup and the separate fixed-order sum
    over the clips of each head, with the reference on."""
    dev = _dev()
    rng = np.random.default_rng(13)
    G, B, T, C, N = 2, 35, 5, 4, 3
    xs = tuple(rng.normal(0.0, 2.0, (B, T, C)).astype(np.float32) for _ in range(G))
    in_len = [int(v) for v in rng.integers(0, T + 1, B)]
    in_len[0] = 0
    pool = [[1], [2, 3], [], [1, 1], [3, 2, 1], [2]]
    lists = tuple([[pool[(b + k + 2 * g) % len(pool)] for k in range(1 + (b + g) % N)] for b in range(B)] for g in range(G))
    refs = [pool[(b + 1) % len(pool)] for b in range(B)]
    loss, det, dxs = _run(xs, in_len, lists, refs, N, T, dev, 1.0, fill=-3, reference=True)
    for g in range(G):
        want = M.mwer(xs[g], in_len, lists[g], refs, 1.0, n_max=N, with_ref=True)
        assert np.abs(want["dlogits"]).max() >= 1e-3 and abs(want["loss"]) > 1e-3
        assert 0 < want["ref_valid"].sum() < B
        _assert_parity(f"G2xB35 head {g}", loss[g], {k: v[g] for k, v in det.items()}, dxs[g], want)


# ------------------------------------------------------------------ 5: the steps
HEADS = ("alignment_gloss_logits", "fuse_coord_gloss_logits")
BEAM, NBEST, WEIGHT, LM_W = NR.MODEL_BEAM, 3, 0.5, 0.5


def _table(fx):
    return NR.random_lm(fx["meta"]["vocab"], seed=5)


def _spec(fx, dev):
    import scattennet_amd as S
    return S.MWER(WEIGHT, beam_size=BEAM, nbest=NBEST, reference=True, head=HEADS, lm=_lm(_table(fx), dev), lm_weight=LM_W)


def _restated(out, src, table):
    """The restatement on the step's own logits, per head, lists from the restatement's search."""
    lens = out["input_lengths"].cpu().numpy()
    lab, ll = src["gloss_labels"].cpu().numpy(), src["gloss_lengths"].cpu().numpy()
    refs = [lab[b, :ll[b]].tolist() for b in range(len(lens))]
    res = []
    for head in HEADS:
        logits = out[head].detach().double().cpu().numpy()
        lists = []
        for b in range(len(logits)):
            entries, gaps = NR.nbest(logits[b], lens[b], BEAM, NBEST, collapse_repeats=False)
            assert min(gaps["frame"], gaps["final"]) >= 1e-4, gaps  # no tie in the search (tests/test_nbest.py)
            lists.append([h for h, _ in entries])
        res.append(M.mwer(logits, lens, lists, refs, 1.0, n_max=NBEST, with_ref=True, lm=table, lm_weight=LM_W))
    return res


@pytest.fixture(scope="module")
def eager(fx):
    """One eager step with the spec and one without on twin models, computed once."""
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev)
    out = S.train_step(model, opt, src, mwer=_spec(fx, dev))
    rep = S.read_report(out)
    with_mwer = ({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in out.items()}, _grads(model), rep)
    plain_model, plain_opt = _trainer(fx, dev)
    plain_out = S.train_step(plain_model, plain_opt, src)
    plain = ({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in plain_out.items()}, _grads(plain_model))
    return {"src": src, "mwer": with_mwer, "plain": plain, "want": _restated(with_mwer[0], src, _table(fx))}


def test_step_losses_and_gradients_against_the_restatement(fx, eager):
    dev = _dev()
    out, grads, rep = eager["mwer"]
    plain_out, plain_grads = eager["plain"]
    want = eager["want"]
    B = len(want[0]["risk"])
    print("mwer_losses", out["mwer_losses"].tolist(), "restated", [w["loss"] for w in want], "ref_valid",
          [w["ref_valid"].tolist() for w in want], "max |dlogits_ref|", [np.abs(w["dlogits"]).max() for w in want])
    assert all(w["ref_valid"].any() and np.abs(w["dlogits"]).max() >= 1e-3 for w in want)  # not a vacuous case
    assert out["mwer_losses"].shape == (2,) and out["mwer_risk"].shape == (2, B) and out["mwer_loss"].dim() == 0
    assert rel_err(out["mwer_losses"], torch.tensor([w["loss"] for w in want])) < TOL
    assert rel_err(out["mwer_risk"], torch.from_numpy(np.stack([w["risk"] for w in want]))) < TOL
    assert rel_err(out["mwer_loss"], torch.tensor(sum(w["loss"] for w in want))) < TOL
    # the parameter gradients minus those of the mwer=None step = WEIGHT * sum_g dlogits_ref through the heads
    model = _build(fx, dev)
    fwd = model(eager["src"])
    torch.autograd.backward([fwd[h] for h in HEADS],
                            [torch.from_numpy(WEIGHT * w["dlogits"]).float().to(dev) for w in want])
    torch.cuda.synchronize()
    ref_grads = _grads(model)
    gscale = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    worst = 0.0
    for k, g in ref_grads.items():
        if g is None:
            continue
        # a parameter the plain step leaves without a gradient has gradient zero there
        mine, plain = (torch.zeros_like(g) if d[k] is None else d[k] for d in (grads, plain_grads))
        diff = mine - plain
        if float(g.abs().max()) >= 1e-4 * gscale:
            worst = max(worst, rel_err(diff, g))
        assert close(diff, g, TOL, gscale), (k, rel_err(diff, g))
    print("parameter gradients: worst rel_err", worst, "gradient scale", gscale)
    assert abs(rep["mwer_loss"] - float(out["mwer_loss"])) == 0.0 and rep["skipped"] is False
    assert abs(rep["mwer_risk"] - float(out["mwer_risk"].mean())) < 1e-6
    assert set(out) - set(plain_out) == {"mwer_loss", "mwer_losses", "mwer_risk", "mwer_report"}


def test_bucketed_step_equals_the_eager_unpadded_step(fx, eager):
    import scattennet_amd as S
    dev = _dev()
    out, grads, rep = eager["mwer"]
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3, mwer=_spec(fx, dev))
    gscale = max(float(g.abs().max()) for g in grads.values() if g is not None)
    for use in ("eager first use", "capture and replay", "replay"):
        got = bts.step(eager["src"])
        got_rep = S.read_report(got)
        torch.cuda.synchronize()
        assert bts.graphs_captured == (0 if use == "eager first use" else 1)
        figs = {k: rel_err(torch.tensor(got_rep[k]), torch.tensor(rep[k])) for k in ("total_loss", "mwer_loss", "mwer_risk")}
        figs["mwer_losses"] = rel_err(got["mwer_losses"], out["mwer_losses"])
        worst = 0.0
        for k, g in grads.items():
            if g is None:
                continue
            mine = model.get_parameter(k).grad.detach().cpu()
            if float(g.abs().max()) >= 1e-4 * gscale:
                worst = max(worst, rel_err(mine, g))
            assert close(mine, g, TOL, gscale), (use, k, rel_err(mine, g))
        print(use, {k: f"{v:.3g}" for k, v in figs.items()}, "gradients worst rel_err", f"{worst:.3g}")
        assert max(figs.values()) < TOL and got_rep["skipped"] is False, (use, figs)
