"""The differentiable head ensemble on the MI355X (scattennet_amd/ensemble.py: EnsembleLogProbsOp,
ensemble_log_probs(..., differentiable=True); csrc/ensemble.hip: sca_ensemble_log_probs_bwd)
against the float64 restatement of tests/ensemble_grad_ref.py, bitwise across its forms (the
detached call, a subset of members, eager / captured), chained with the MWER and the CTC loss,
and as the head of MWER in the training steps on tests/golden/model_small.

Bound: golden_util.rel_err(got, want) < 1e-3 per member tensor, the project's.  Every test prints
the figure it asserts.  Worst measured values on one MI355X: member gradients against
the restatement 1.05e-6 over all parity cases; through the MWER loss 2.9e-6 and through the CTC
loss 1.6e-6; G = 1 against float64 log_softmax 9.6e-8; the steps' parameter gradients 0 against
the step composed by hand (the same kernels on the same bits) and 1.2e-5 bucketed against eager."""
import functools

import numpy as np
import pytest
import torch

from tests import ensemble_grad_ref as GR
from tests import ensemble_ref as R
from tests import mwer_ref as M
from tests import nbest_ref as NR
from tests.golden_util import close, rel_err
from tests.mwer_gpu import fx  # noqa: F401  (the fixture, by name)
from tests.mwer_gpu import TOL, _bits, _build, _dev, _grads, _nbest, _trainer

pytestmark = pytest.mark.gpu

# (G, B, T, C): C below a wave; C % 4 != 0; C % 64 != 0; 1, 3, 14, 15 rows (not a multiple of the
# four rows per workgroup); G = 1 and 8; the evaluation shape
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (3, 2, 7, 70), (5, 3, 5, 33), (8, 1, 3, 1124), (2, 8, 64, 1124)]
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
CLAMPED = {(3, 2, 7, 70), (2, 8, 64, 1124)}  # these also hold the +-50 rows (ensemble_ref.case)
MEMBERS = ("left", "right", "body")
BEAM, NBEST, WEIGHT = NR.MODEL_BEAM, 3, 0.5
MWER_SHAPE = (5, 16, 4, 8, 8)  # (B, T, C, W, N) of tests/mwer_ref.py


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(inputs, dout, {(weighted, mode): the restatement's G gradients}), computed once per shape."""
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    dout = GR.dout_of(shape[1:])
    refs = {(wt, mode): GR.vjp(xs, R.cycled_weights(shape[0]) if wt else None, mode, dout)
            for wt in (False, True) for mode in R.MODES}
    return xs, dout, refs


def _leaves(xs, dev):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev).requires_grad_(True) for x in xs]


def _backward(xd, weights, mode, dout):
    """The members' gradients of the differentiable call under the incoming gradient dout."""
    import scattennet_amd as S
    for x in xd:
        x.grad = None
    out = S.ensemble_log_probs(xd, weights, mode, differentiable=True)
    out.backward(dout)
    return out.detach(), [x.grad for x in xd]


# ------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_member_gradients_against_the_restatement(shape):
    dev = _dev()
    xs, dout, refs = _case(shape)
    xd, dd = _leaves(xs, dev), torch.from_numpy(dout).to(dev)
    for (weighted, mode), want in refs.items():
        out, grads = _backward(xd, R.cycled_weights(shape[0]) if weighted else None, mode, dd)
        assert out.shape == xd[0].shape
        for g, (got, ref) in enumerate(zip(grads, want)):
            assert got.shape == xd[g].shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
            err = rel_err(got, torch.from_numpy(ref))
            print(f"{IDS[SHAPES.index(shape)]} {mode} weighted={weighted} member {g}: rel_err {err:.3e}")
            assert err < TOL, (mode, weighted, g, err)


def test_a_member_off_the_16_byte_boundary_takes_the_scalar_path():
    """C % 4 == 0 and every other row aligned: member 1 is a view one float into a larger buffer."""
    dev = _dev()
    shape = (3, 2, 5, 64)
    xs = R.case(*shape)
    dout = GR.dout_of(shape[1:])
    dd = torch.from_numpy(dout).to(dev)
    aligned = _leaves(xs, dev)
    buf = torch.zeros(xs[1].size + 1, device=dev)
    buf[1:].copy_(torch.from_numpy(xs[1]).to(dev).reshape(-1))
    view = buf[1:].view(xs[1].shape).requires_grad_(True)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and aligned[1].data_ptr() % 16 == 0
    for mode in R.MODES:
        want = GR.vjp(xs, R.cycled_weights(3), mode, dout)
        out_a, ga = _backward(aligned, R.cycled_weights(3), mode, dd)
        ga = [g.clone() for g in ga]
        out_v, gv = _backward([aligned[0], view, aligned[2]], R.cycled_weights(3), mode, dd)
        for g in range(3):
            err = rel_err(gv[g], torch.from_numpy(want[g]))
            print(f"misaligned member, {mode}, member {g}: rel_err {err:.3e}; against the 16-byte path "
                  f"{rel_err(gv[g], ga[g]):.3e}")
            assert err < TOL and rel_err(ga[g], torch.from_numpy(want[g])) < TOL, (mode, g, err)
        assert rel_err(out_v, out_a) < TOL


# ------------------------------------------------------------------ 2, 3: bitwise forms
def test_differentiable_output_is_bitwise_the_default_call():
    import scattennet_amd as S
    dev = _dev()
    for shape in ((3, 2, 7, 70), (5, 3, 5, 33), (2, 8, 64, 1124)):
        xd = _leaves(R.case(*shape, clamp_rows=shape in CLAMPED), dev)
        w = R.cycled_weights(shape[0])
        for mode in R.MODES:
            plain = S.ensemble_log_probs(xd, w, mode)
            diff = S.ensemble_log_probs(xd, w, mode, differentiable=True)
            assert not plain.requires_grad and diff.requires_grad and diff.grad_fn is not None
            assert torch.equal(_bits(plain), _bits(diff.detach())), (shape, mode)
            print(shape, mode, "bitwise equal:", True)
        frozen = [x.detach() for x in xd]  # no member requires a gradient: a plain tensor comes back
        assert not S.ensemble_log_probs(frozen, w, "prob", differentiable=True).requires_grad


def test_only_the_members_that_require_a_gradient_receive_one():
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs, dout, _ = _case(shape)
    dd = torch.from_numpy(dout).to(dev)
    for mode in R.MODES:
        _, all_grads = _backward(_leaves(xs, dev), R.cycled_weights(3), mode, dd)
        some = _leaves(xs, dev)
        some[1] = some[1].detach()
        _, grads = _backward(some, R.cycled_weights(3), mode, dd)
        assert some[1].grad is None and grads[1] is None
        for g in (0, 2):
            same = torch.equal(_bits(grads[g]), _bits(all_grads[g]))
            print(mode, "member", g, "bitwise the all-members call:", same)
            assert same and float(grads[g].abs().max()) > 0


# ------------------------------------------------------------------ 4: one member
def test_one_member_is_the_log_softmax_backward():
    dev = _dev()
    for shape in ((1, 1, 1, 2), (1, 3, 5, 33), (1, 2, 7, 1124)):
        x = R.case(*shape)[0]
        dd = torch.from_numpy(GR.dout_of(shape[1:])).to(dev)
        t = torch.from_numpy(x).to(dev).requires_grad_(True)
        torch.log_softmax(t, -1).backward(dd)
        t64 = torch.from_numpy(x).double().requires_grad_(True)
        torch.log_softmax(t64, -1).backward(dd.cpu().double())
        for mode in R.MODES:
            _, (got,) = _backward(_leaves([x], dev), [2.5], mode, dd)
            err, err64 = rel_err(got, t.grad), rel_err(got, t64.grad)
            print(shape, mode, f"against torch on the device {err:.3e}, against float64 {err64:.3e}")
            assert err < TOL and err64 < TOL, (shape, mode, err, err64)


# ------------------------------------------------------------------ 5: rows without a gradient
def test_rows_with_zero_incoming_gradient_get_zero_gradients():
    dev = _dev()
    for shape, zero in (((3, 2, 7, 70), 5), ((2, 3, 5, 64), 6), ((5, 3, 5, 33), 1)):
        xs = R.case(*shape, clamp_rows=shape in CLAMPED)
        dd = torch.from_numpy(GR.dout_of(shape[1:], zero_rows=zero)).to(dev)
        for mode in R.MODES:
            _, grads = _backward(_leaves(xs, dev), R.cycled_weights(shape[0]), mode, dd)
            for g, dx in enumerate(grads):
                rows = dx.reshape(-1, shape[-1])
                worst = float(rows[-zero:].abs().max())
                print(shape, mode, "member", g, "max |dx| over the rows with dout == 0:", worst)
                assert bool((rows[-zero:] == 0).all()) and float(rows[:-zero].abs().max()) > 0


# ------------------------------------------------------------------ 6: capture
def test_captured_forward_and_backward_replay_bitwise():
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs = _leaves(R.case(*shape, clamp_rows=True), dev)
    w = R.cycled_weights(3)
    dd = torch.from_numpy(GR.dout_of(shape[1:])).to(dev)

    def chain():
        res = []
        for mode in R.MODES:
            for x in xs:
                x.grad = None
            out = S.ensemble_log_probs(xs, w, mode, differentiable=True)
            out.backward(dd)
            res += [out.detach()] + [x.grad for x in xs]
        return res

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for seed in (None, 5):  # the captured inputs, then refilled ones
        if seed is not None:
            with torch.no_grad():
                for x, new in zip(xs, R.case(*shape, seed=seed)):
                    x.copy_(torch.from_numpy(new))
                dd.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)
        assert all(float(t.abs().max()) > 0 for t in got)
        print("replay with seed", seed, "bitwise the eager chain:", True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_reduced_precision_members_receive_gradients_in_their_dtype(dtype):
    dev = _dev()
    shape = (3, 2, 7, 70)
    low = [torch.from_numpy(x).to(dev).to(dtype) for x in R.case(*shape)]
    dd = torch.from_numpy(GR.dout_of(shape[1:])).to(dev)
    for mode in R.MODES:
        out32, want = _backward([x.float().requires_grad_(True) for x in low], [1, 2, 3], mode, dd)
        leaves = [x.clone().requires_grad_(True) for x in low]
        out, grads = _backward(leaves, [1, 2, 3], mode, dd.to(dtype))
        assert out.dtype == dtype and torch.equal(out, out32.to(dtype))
        # the incoming gradient is rounded to the members' dtype first: the bound is that rounding's
        _, want_low = _backward([x.float().requires_grad_(True) for x in low], [1, 2, 3], mode, dd.to(dtype).float())
        for g in range(3):
            assert grads[g].dtype == dtype and torch.equal(grads[g], want_low[g].to(dtype)), (mode, g)
            print(dtype, mode, "member", g, "rel_err against the fp32 gradients", f"{rel_err(grads[g], want[g]):.3e}")


# ------------------------------------------------------------------ 7, 8: chained with the losses
@functools.lru_cache(maxsize=None)
def _members():
    """Case MWER_SHAPE of tests/mwer_ref.py and two more member tensors from other seeds."""
    logits, in_len, lists, refs = M.case_inputs_ext(MWER_SHAPE)
    B, T, C = MWER_SHAPE[:3]
    more = [np.random.default_rng(s).normal(0.0, 2.0, (B, T, C)).astype(np.float32) for s in (21, 22)]
    return [np.asarray(logits, np.float32)] + more, list(in_len), lists, refs


@pytest.mark.parametrize("mode", R.MODES)
def test_mwer_on_the_ensemble_against_the_restatements(mode):
    import scattennet_amd as S
    dev = _dev()
    xs, in_len, lists, refs = _members()
    B, T, C, W, N = MWER_SHAPE
    w = R.cycled_weights(3)
    ens = R.ensemble(xs, w, mode)
    want = M.mwer(ens, in_len, lists, refs, M.POSTERIOR_SCALE, n_max=N, with_ref=True)
    want_dx = GR.vjp(xs, w, mode, want["dlogits"])
    print(mode, "max |dloss / d ensemble| of the restatement", np.abs(want["dlogits"]).max(), "per member",
          [float(np.abs(d).max()) for d in want_dx])
    assert np.abs(want["dlogits"]).max() >= 1e-3 and all(np.abs(d).max() >= 1e-3 for d in want_dx)  # not vacuous
    xd = _leaves(xs, dev)
    ref, ref_len = M.pack_refs(refs)
    loss, det = S.mwer_loss(S.ensemble_log_probs(xd, w, mode, differentiable=True), torch.tensor(in_len),
                            torch.from_numpy(ref), torch.from_numpy(ref_len), nbest=_nbest(lists, N, T, dev),
                            posterior_scale=M.POSTERIOR_SCALE, return_details=True, reference=True)
    loss.backward()
    torch.cuda.synchronize()
    ll, wl = det["loglik"].double().cpu().numpy(), want["loglik"]
    assert np.array_equal(np.isneginf(ll), np.isneginf(wl))
    fin = np.isfinite(wl)
    figs = {"loss": rel_err(loss, torch.tensor(want["loss"])),
            "loglik": rel_err(torch.from_numpy(ll[fin]), torch.from_numpy(wl[fin])),
            "posterior": rel_err(det["posterior"], torch.from_numpy(want["posterior"])),
            "risk": rel_err(det["risk"], torch.from_numpy(want["risk"]))}
    for g in range(3):
        figs[f"dx{g}"] = rel_err(xd[g].grad, torch.from_numpy(want_dx[g]))
    print(mode, {k: f"{v:.3g}" for k, v in figs.items()}, "loss", want["loss"])
    assert np.array_equal(det["errors"].cpu().numpy().astype(np.int64), want["errors"])
    assert np.array_equal(det["ref_valid"].cpu().numpy().astype(np.int64), want["ref_valid"])
    assert max(figs.values()) < TOL, figs


@pytest.mark.parametrize("mode", R.MODES)
def test_ctc_loss_on_the_ensemble_against_float64_torch(mode):
    """CTCLossOp on the op's output, over the clips whose reference is not empty and has a path
    (in_len >= len + repeats: there the loss's rule T_b = max(in_len, 1, S_b) changes nothing)."""
    import scattennet_amd as S
    from scattennet_amd.heads import CTCLossOp
    dev = _dev()
    xs, in_len, _, refs = _members()
    fit = [b for b in range(len(refs)) if refs[b] and M.fits(refs[b], in_len[b])]
    assert len(fit) >= 2
    xs = [x[fit] for x in xs]
    refs, in_len = [refs[b] for b in fit], [in_len[b] for b in fit]
    w = R.cycled_weights(3)
    ref, ref_len = M.pack_refs(refs)
    # float64 torch: ctc_loss on the composition, the mean over the clips as compute_loss takes it
    ts = [torch.from_numpy(x).double().requires_grad_(True) for x in xs]
    wn = torch.tensor(R.normalised(w, 3))
    lps = [torch.log_softmax(t, -1) for t in ts]
    comp = torch.logsumexp(torch.stack([lp + torch.log(wn[g]) for g, lp in enumerate(lps)]), 0) if mode == "prob" \
        else torch.log_softmax(sum(wn[g] * lp for g, lp in enumerate(lps)), -1)
    nll = torch.nn.functional.ctc_loss(M.log_probs(comp).transpose(0, 1), torch.from_numpy(ref).long(),
                                       torch.tensor(in_len), torch.from_numpy(ref_len).long(), blank=0, reduction="none")
    assert bool(torch.isfinite(nll).all()) and float(nll.detach().mean()) < 100.0
    nll.mean().backward()
    xd = _leaves(xs, dev)
    loss, _ = CTCLossOp.apply(S.ensemble_log_probs(xd, w, mode, differentiable=True), torch.from_numpy(ref).to(dev),
                              torch.tensor(in_len, dtype=torch.int32, device=dev), torch.from_numpy(ref_len).to(dev))
    loss.backward()
    torch.cuda.synchronize()
    figs = {"loss": rel_err(loss, nll.mean())}
    for g in range(3):
        assert float(ts[g].grad.abs().max()) >= 1e-3
        figs[f"dx{g}"] = rel_err(xd[g].grad, ts[g].grad)
    print(mode, "clips", fit, {k: f"{v:.3g}" for k, v in figs.items()}, "loss", float(nll.detach().mean()))
    assert max(figs.values()) < TOL, figs


# ------------------------------------------------------------------ 9, 10: the steps
def _head(kind):
    import scattennet_amd as S
    spec = S.EnsembleSpec(MEMBERS, mode="logprob" if kind == "logprob" else "prob")
    return ("fuse_coord_gloss_logits", spec) if kind == "key+prob" else spec


def _mwer(kind):
    import scattennet_amd as S
    return S.MWER(WEIGHT, BEAM, NBEST, reference=True, head=_head(kind))


@pytest.fixture(scope="module")
def plain(fx):
    """The mwer=None step's gradients, once."""
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev)
    S.train_step(model, opt, src)
    torch.cuda.synchronize()
    return src, _grads(model)


def _by_hand(fx, src, kind):
    """The step composed from the public calls on a twin model: (mwer losses, gradients)."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    out = model(src)
    head = _head(kind)
    tensors = [out[h] if isinstance(h, str) else
               S.ensemble_log_probs([out[k] for k in h.members], h.weights, h.mode, differentiable=True)
               for h in (head if isinstance(head, tuple) else (head,))]
    loss = S.mwer_loss(tensors if isinstance(head, tuple) else tensors[0], out["input_lengths"], src["gloss_labels"],
                       src["gloss_lengths"], beam_size=BEAM, nbest_size=NBEST, reference=True)
    (out["total_loss"] + WEIGHT * loss.sum()).backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), _grads(model)


def _compare(where, grads, want):
    gscale = max(float(g.abs().max()) for g in want.values() if g is not None)
    worst = 0.0
    for k, g in want.items():
        if g is None:
            assert grads[k] is None, (where, k)
            continue
        if float(g.abs().max()) >= 1e-4 * gscale:
            worst = max(worst, rel_err(grads[k], g))
        assert close(grads[k], g, TOL, gscale), (where, k, rel_err(grads[k], g))
    print(where, "parameter gradients: worst rel_err", f"{worst:.3g}", "gradient scale", gscale)
    return worst


@pytest.mark.parametrize("kind", ["prob", "logprob", "key+prob"])
def test_train_step_with_an_ensemble_head_equals_the_step_composed_by_hand(fx, plain, kind):
    import scattennet_amd as S
    dev = _dev()
    src, plain_grads = plain
    model, opt = _trainer(fx, dev)
    out = S.train_step(model, opt, src, mwer=_mwer(kind))
    rep = S.read_report(out)
    torch.cuda.synchronize()
    grads = _grads(model)
    want_loss, want = _by_hand(fx, src, kind)
    print(kind, "mwer_loss", rep["mwer_loss"], "by hand", want_loss.tolist(), "skipped", rep["skipped"])
    assert rep["skipped"] is False and np.isfinite(rep["mwer_loss"])
    if kind == "key+prob":
        assert out["mwer_losses"].shape == (2,) and out["mwer_risk"].shape[0] == 2
        assert rel_err(out["mwer_losses"], want_loss) < TOL
    else:
        assert "mwer_losses" not in out and out["mwer_loss"].dim() == 0
    assert rel_err(out["mwer_loss"], want_loss.sum()) < TOL
    _compare(kind, grads, want)
    # the term reaches the members: the gradients are not the mwer=None step's
    differs = [k for k, g in grads.items() if g is not None and plain_grads[k] is not None and
               not torch.equal(g, plain_grads[k])]
    gscale = max(float(g.abs().max()) for g in plain_grads.values() if g is not None)
    delta = max(float((grads[k] - plain_grads[k]).abs().max()) for k in differs)
    print(kind, len(differs), "parameter gradients differ from the mwer=None step, by up to", delta, "of", gscale)
    assert differs and delta >= 1e-3 * gscale


def test_bucketed_step_with_an_ensemble_head_equals_the_eager_unpadded_step(fx, plain):
    import scattennet_amd as S
    dev = _dev()
    src, _ = plain
    eager_model, eager_opt = _trainer(fx, dev)
    eager_out = S.train_step(eager_model, eager_opt, src, mwer=_mwer("key+prob"))
    rep = S.read_report(eager_out)
    torch.cuda.synchronize()
    want = _grads(eager_model)
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3, mwer=_mwer("key+prob"))
    for use in ("eager first use", "capture and replay", "replay"):
        got = bts.step(src)
        got_rep = S.read_report(got)
        torch.cuda.synchronize()
        assert bts.graphs_captured == (0 if use == "eager first use" else 1)
        figs = {k: rel_err(torch.tensor(got_rep[k]), torch.tensor(rep[k])) for k in ("total_loss", "mwer_loss", "mwer_risk")}
        figs["mwer_losses"] = rel_err(got["mwer_losses"], eager_out["mwer_losses"])
        print(use, {k: f"{v:.3g}" for k, v in figs.items()})
        _compare(use, _grads(model), want)
        assert max(figs.values()) < TOL and got_rep["skipped"] is False, (use, figs)
