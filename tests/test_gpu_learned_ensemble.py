"""The learned head ensemble on the MI355X (scattennet_amd/ensemble.py: LearnedEnsemble,
LearnedEnsembleLogProbsOp, ensemble_log_probs(weight_logits=...); csrc/ensemble.hip:
sca_ensemble_log_probs_dw / _dw_bwd) against the float64 restatement of
tests/ensemble_weight_ref.py, its structural properties, bitwise under capture while theta changes
in place, and in the training and evaluation steps on tests/golden/model_small.

Bound: golden_util.rel_err(got, want) < 1e-3 per tensor, the project's.  Every test prints the
figure it asserts.  Worst measured values on one MI355X: out 1.8e-7, member
gradients 1.05e-6 and d theta 1.03e-6 against the restatement over all parity cases,
|sum_g d theta_g| / max 2.6e-6; freeze() against the learned call 1.6e-7; the train step against
the step composed by hand 0 (the same kernels on the same bits); the bucketed padded step's
d theta against the eager unpadded one 6.5e-7."""
import functools

import numpy as np
import pytest
import torch

from tests import ensemble_grad_ref as GR
from tests import ensemble_ref as R
from tests import ensemble_weight_ref as WR
from tests import nbest_ref as NR
from tests.golden_util import rel_err
from tests.mwer_gpu import fx  # noqa: F401  (the fixture, by name)
from tests.mwer_gpu import ADAM, TOL, _bits, _build, _dev, _grads, _trainer
from tests.test_gpu_ensemble_backward import _compare, _leaves

pytestmark = pytest.mark.gpu

# (G, B, T, C): G = 1; C below a wave; the clamp rows; the scalar path (C % 4 != 0); full G on the
# 16-byte path; 265 rows, so the summing launch's per-thread loop takes a second trip.  15, 14, 18
# and 3 rows leave partly empty workgroups.
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (3, 2, 7, 70), (5, 2, 9, 33), (8, 1, 3, 1124), (2, 5, 53, 8)]
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
CLAMPED = {(3, 2, 7, 70)}
MEMBERS = ("left", "right", "body")
BEAM, NBEST, WEIGHT = NR.MODEL_BEAM, 3, 0.5
ENS = "learned_gloss_logits"


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(inputs, theta, dout, {mode: (out, the G gradients, d theta) of the restatement}), once per shape."""
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    theta = WR.theta_of(shape[0]).astype(np.float32)
    dout = GR.dout_of(shape[1:])
    refs = {mode: (WR.ensemble(xs, theta, mode),) + WR.vjp(xs, theta, mode, dout) for mode in R.MODES}
    return xs, theta, dout, refs


def _theta(theta, dev, grad=True):
    return torch.from_numpy(np.asarray(theta, np.float32)).to(dev).requires_grad_(grad)


def _backward(xd, th, mode, dout):
    """(out, the members' gradients, d theta) of the differentiable call under dout."""
    import scattennet_amd as S
    for t in list(xd) + [th]:
        t.grad = None
    out = S.ensemble_log_probs(xd, None, mode, weight_logits=th, differentiable=True)
    out.backward(dout)
    return out.detach(), [x.grad for x in xd], th.grad


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_outputs_and_gradients_against_the_restatement(shape):
    dev = _dev()
    G = shape[0]
    xs, theta, dout, refs = _case(shape)
    xd, th, dd = _leaves(xs, dev), _theta(theta, dev), torch.from_numpy(dout).to(dev)
    for mode, (want_out, want_dx, want_dt) in refs.items():
        out, grads, dt = _backward(xd, th, mode, dd)
        assert out.shape == xd[0].shape and dt.shape == (G,) and dt.dtype == torch.float32
        assert bool(torch.isfinite(dt).all())
        figs = {"out": rel_err(out, torch.from_numpy(want_out))}
        for g in range(G):
            figs[f"dx{g}"] = rel_err(grads[g], torch.from_numpy(want_dx[g]))
        if G == 1:
            assert bool((dt == 0).all())
        else:
            figs["dtheta"] = rel_err(dt, torch.from_numpy(want_dt))
            figs["sum/max"] = abs(float(dt.double().sum())) / float(dt.abs().max())
        print(IDS[SHAPES.index(shape)], mode, {k: f"{v:.3e}" for k, v in figs.items()},
              "max |dtheta| of the restatement", float(np.abs(want_dt).max()))
        assert max(figs.values()) < TOL, (mode, figs)


def test_a_member_off_the_16_byte_boundary_takes_the_scalar_path():
    """C % 4 == 0 and every other row aligned: member 1 is a view one float into a larger buffer."""
    dev = _dev()
    shape = (3, 2, 5, 64)
    xs = R.case(*shape)
    theta = WR.theta_of(3).astype(np.float32)
    dout = GR.dout_of(shape[1:])
    dd, th = torch.from_numpy(dout).to(dev), _theta(theta, dev)
    aligned = _leaves(xs, dev)
    buf = torch.zeros(xs[1].size + 1, device=dev)
    buf[1:].copy_(torch.from_numpy(xs[1]).to(dev).reshape(-1))
    view = buf[1:].view(xs[1].shape).requires_grad_(True)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and aligned[1].data_ptr() % 16 == 0
    for mode in R.MODES:
        want_dx, want_dt = WR.vjp(xs, theta, mode, dout)
        out_a, ga, ta = _backward(aligned, th, mode, dd)
        ga, ta = [g.clone() for g in ga], ta.clone()
        out_v, gv, tv = _backward([aligned[0], view, aligned[2]], th, mode, dd)
        figs = {"dtheta": rel_err(tv, torch.from_numpy(want_dt)), "dtheta 16-byte": rel_err(ta, torch.from_numpy(want_dt)),
                "out": rel_err(out_v, out_a)}
        for g in range(3):
            figs[f"dx{g}"] = rel_err(gv[g], torch.from_numpy(want_dx[g]))
        print("misaligned member,", mode, {k: f"{v:.3e}" for k, v in figs.items()})
        assert max(figs.values()) < TOL, (mode, figs)


# ------------------------------------------------------------------ structural properties
def test_one_member_has_an_exactly_zero_weight_gradient():
    dev = _dev()
    for shape in ((1, 1, 1, 2), (1, 3, 5, 33), (1, 2, 7, 1124)):
        x = R.case(*shape)
        dd = torch.from_numpy(GR.dout_of(shape[1:])).to(dev)
        for mode in R.MODES:
            out, (dx,), dt = _backward(_leaves(x, dev), _theta([2.5], dev), mode, dd)
            # theta alone: the memset is all the call does
            th = _theta([2.5], dev)
            _backward([t.detach() for t in _leaves(x, dev)], th, mode, dd)
            err = rel_err(out, torch.from_numpy(R.log_softmax(x[0])))
            print(shape, mode, "dtheta", dt.tolist(), th.grad.tolist(), f"out against log_softmax {err:.3e}")
            assert dt.shape == (1,) and bool((dt == 0).all()) and bool((th.grad == 0).all())
            assert err < TOL and float(dx.abs().max()) > 0


def test_rows_with_zero_incoming_gradient_contribute_exactly_zero():
    """d theta with the last five rows of dout at zero is bitwise the same whatever the members
    hold in those rows, and equals d theta of the tensors without those rows."""
    dev = _dev()
    for shape in ((3, 2, 7, 70), (2, 5, 53, 8), (5, 2, 9, 33)):
        G, B, T, C = shape
        xs = R.case(*shape, clamp_rows=shape in CLAMPED)
        theta = WR.theta_of(G).astype(np.float32)
        dout = GR.dout_of(shape[1:], zero_rows=5)
        other = [x.copy() for x in xs]
        for x in other:
            x.reshape(-1, C)[-5:] += 1.5
        cut = [np.ascontiguousarray(x.reshape(1, -1, C)[:, :-5]) for x in xs]
        dd = torch.from_numpy(dout).to(dev)
        for mode in R.MODES:
            _, _, dt = _backward(_leaves(xs, dev), _theta(theta, dev), mode, dd)
            _, _, dt_other = _backward(_leaves(other, dev), _theta(theta, dev), mode, dd)
            _, _, dt_cut = _backward(_leaves(cut, dev), _theta(theta, dev), mode,
                                     dd.reshape(1, -1, C)[:, :-5].contiguous())
            err = rel_err(dt, torch.from_numpy(WR.dtheta(xs, theta, mode, dout)))
            print(shape, mode, "dtheta", dt.tolist(), "bitwise with other members in the zero rows:",
                  torch.equal(_bits(dt), _bits(dt_other)), "equal without the rows:", torch.equal(dt, dt_cut),
                  f"rel_err {err:.3e}")
            assert torch.equal(_bits(dt), _bits(dt_other)) and torch.equal(dt, dt_cut)
            assert err < TOL and float(dt.abs().max()) > 0


def test_only_what_requires_a_gradient_receives_one():
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs, theta, dout, refs = _case(shape)
    dd = torch.from_numpy(dout).to(dev)
    for mode in R.MODES:
        _, all_dx, all_dt = _backward(_leaves(xs, dev), _theta(theta, dev), mode, dd)
        all_dx, all_dt = [g.clone() for g in all_dx], all_dt.clone()
        # theta alone: in "prob" s_g is still formed for the members, whose entries are all null
        frozen = [x.detach() for x in _leaves(xs, dev)]
        out, dx, dt = _backward(frozen, _theta(theta, dev), mode, dd)
        assert dx == [None] * 3 and out.shape == frozen[0].shape
        err = rel_err(dt, torch.from_numpy(refs[mode][2]))
        print(mode, "theta alone: bitwise the all-gradients call", torch.equal(_bits(dt), _bits(all_dt)), f"rel_err {err:.3e}")
        assert torch.equal(_bits(dt), _bits(all_dt)) and err < TOL
        # the members alone
        th = _theta(theta, dev, grad=False)
        _, dx, dt = _backward(_leaves(xs, dev), th, mode, dd)
        assert dt is None and th.grad is None
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(dx, all_dx))
        # a subset: members 0 and 2 with theta
        some = _leaves(xs, dev)
        some[1] = some[1].detach()
        _, dx, dt = _backward(some, _theta(theta, dev), mode, dd)
        assert dx[1] is None and torch.equal(_bits(dt), _bits(all_dt))
        assert torch.equal(_bits(dx[0]), _bits(all_dx[0])) and torch.equal(_bits(dx[2]), _bits(all_dx[2]))
        # nothing requires a gradient: a plain tensor comes back
        import scattennet_amd as S
        plain = S.ensemble_log_probs(frozen, None, mode, weight_logits=th, differentiable=True)
        assert not plain.requires_grad and torch.equal(_bits(plain), _bits(out))
        print(mode, "members alone, subset, none: as the all-gradients call")


def test_frozen_host_weights_agree_with_the_learned_ensemble():
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs, theta, dout, _ = _case(shape)
    dd = torch.from_numpy(dout).to(dev)
    outputs = dict(zip(MEMBERS, _leaves(xs, dev)))
    for mode in R.MODES:
        ens = S.LearnedEnsemble(MEMBERS, mode, init=R.cycled_weights(3)).to(dev)
        spec = ens.freeze()
        assert spec.weights == pytest.approx(tuple(WR.softmax_weights(theta)), abs=1e-6)
        for x in outputs.values():
            x.grad = None
        learned = ens.compute(outputs, differentiable=True)
        learned.backward(dd)
        got = [outputs[k].grad.clone() for k in MEMBERS]
        for x in outputs.values():
            x.grad = None
        fixed = spec.compute(outputs, differentiable=True)
        fixed.backward(dd)
        figs = {"out": rel_err(learned, fixed), "detached": rel_err(ens.compute(outputs), spec.compute(outputs))}
        for g, k in enumerate(MEMBERS):
            figs[f"dx{g}"] = rel_err(got[g], outputs[k].grad)
        print(mode, "learned against freeze()", {k: f"{v:.3e}" for k, v in figs.items()})
        assert max(figs.values()) < TOL and ens.weight_logits.grad is not None


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_reduced_precision_weight_logits_receive_their_gradient_in_their_dtype(dtype):
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs, theta, dout, _ = _case(shape)
    dd = torch.from_numpy(dout).to(dev)
    low = torch.from_numpy(theta).to(dev).to(dtype)
    for mode in R.MODES:
        out32, _, want = _backward(_leaves(xs, dev), low.float().requires_grad_(True), mode, dd)
        th = low.clone().requires_grad_(True)
        out, _, dt = _backward(_leaves(xs, dev), th, mode, dd)
        print(dtype, mode, "dtheta", dt.tolist(), "fp32", want.tolist())
        assert dt.dtype == dtype and torch.equal(dt, want.to(dtype)) and torch.equal(_bits(out), _bits(out32))


# ------------------------------------------------------------------ capture
def test_captured_forward_and_backward_follow_theta_without_recapture():
    """The weights are read from device memory, so a replay after theta.copy_(new) is bitwise the
    eager call at new.  With weights in the kernel arguments the replay would repeat the first."""
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 2, 7, 70)
    xs = _leaves(R.case(*shape, clamp_rows=True), dev)
    th = _theta(WR.theta_of(3), dev)
    dd = torch.from_numpy(GR.dout_of(shape[1:])).to(dev)

    def chain():
        res = []
        for mode in R.MODES:
            for t in xs + [th]:
                t.grad = None
            out = S.ensemble_log_probs(xs, None, mode, weight_logits=th, differentiable=True)
            out.backward(dd)
            res += [out.detach()] + [x.grad for x in xs] + [th.grad]
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
    replays = []
    for new in (None, [0.7, -1.1, 0.2]):
        if new is not None:
            with torch.no_grad():
                th.copy_(torch.tensor(new))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (new, i)
        assert all(float(t.abs().max()) > 0 for t in got)
        print("replay at theta =", th.tolist(), "bitwise the eager chain:", True)
        replays.append(got)
    differ = [not torch.equal(a, b) for a, b in zip(*replays)]
    print("tensors that differ between the two replays:", sum(differ), "of", len(differ))
    assert all(differ)


# ------------------------------------------------------------------ the steps
def _learned(dev, mode="prob"):
    import scattennet_amd as S
    return S.LearnedEnsemble(MEMBERS, mode, init=[1.0, 2.0, 0.5]).to(dev)


def _mwer(ens):
    import scattennet_amd as S
    return S.MWER(WEIGHT, BEAM, NBEST, reference=True, head=("fuse_coord_gloss_logits", ens))


def _src(fx, dev):
    return {k: v.to(dev) for k, v in fx["in"].items()}


def _trainer_with(fx, dev, ens, **adam):
    import scattennet_amd as S
    model = _build(fx, dev)
    return model, S.FusedAdam(list(model.parameters()) + list(ens.parameters()), **{**ADAM, **adam})


@pytest.mark.parametrize("mode", R.MODES)
def test_train_step_with_a_learned_ensemble_equals_the_step_composed_by_hand(fx, mode):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    ens = _learned(dev, mode)
    model, opt = _trainer_with(fx, dev, ens)  # lr 0: both steps see the same parameters
    out = S.train_step(model, opt, src, mwer=_mwer(ens))
    rep = S.read_report(out)
    torch.cuda.synchronize()
    first = ens.weight_logits.grad.clone()
    # by hand, on a twin
    twin_ens = _learned(dev, mode)
    twin = _build(fx, dev)
    o = twin(src)
    e = S.ensemble_log_probs([o[k] for k in MEMBERS], None, mode, weight_logits=twin_ens.weight_logits, differentiable=True)
    loss = S.mwer_loss([o["fuse_coord_gloss_logits"], e], o["input_lengths"], src["gloss_labels"], src["gloss_lengths"],
                       beam_size=BEAM, nbest_size=NBEST, reference=True)
    (o["total_loss"] + WEIGHT * loss.sum()).backward()
    torch.cuda.synchronize()
    want = twin_ens.weight_logits.grad
    figs = {"mwer_losses": rel_err(out["mwer_losses"], loss), "dtheta": rel_err(first, want)}
    print(mode, {k: f"{v:.3g}" for k, v in figs.items()}, "dtheta", first.tolist(), "by hand", want.tolist(),
          "mwer_loss", rep["mwer_loss"])
    assert rep["skipped"] is False and max(figs.values()) < TOL and float(want.abs().max()) > 0
    _compare(mode, _grads(model), _grads(twin))
    # a second step: the gradient is that step's alone, not the sum of both
    S.train_step(model, opt, src, mwer=_mwer(ens))
    torch.cuda.synchronize()
    second = ens.weight_logits.grad
    print(mode, "after two steps", second.tolist(), "against one step's", rel_err(second, first))
    assert rel_err(second, first) < TOL


def test_the_update_moves_theta_and_the_finite_guard_holds_it(fx):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    ens = _learned(dev)
    model, opt = _trainer_with(fx, dev, ens, lr=1e-2)
    before = ens.weight_logits.detach().clone()
    S.read_report(S.train_step(model, opt, src, mwer=_mwer(ens)))
    moved = ens.weight_logits.detach().clone()
    step = float((moved - before).abs().max())
    print("theta", before.tolist(), "->", moved.tolist(), "largest move", step)
    assert bool(torch.isfinite(moved).all()) and 1e-3 < step < 2e-2  # Adam's first step: lr per element
    # a non-finite guard skips the 3-float tensor like every other parameter
    opt.step(loss=torch.full((), float("nan"), device=dev))
    torch.cuda.synchronize()
    assert int(opt.skipped) == 1 and torch.equal(_bits(ens.weight_logits.detach()), _bits(moved))
    # the reference checkpoint still loads strictly: the module is outside the model
    model.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)


def test_bucketed_step_on_a_padded_batch_gives_the_unpadded_weight_gradient(fx):
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    eager_ens = _learned(dev)
    eager_model, eager_opt = _trainer_with(fx, dev, eager_ens)
    rep = S.read_report(S.train_step(eager_model, eager_opt, src, mwer=_mwer(eager_ens)))
    torch.cuda.synchronize()
    want, want_grads = eager_ens.weight_logits.grad.clone(), _grads(eager_model)
    ens = _learned(dev)
    model, opt = _trainer_with(fx, dev, ens)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3, mwer=_mwer(ens))
    for use in ("eager first use", "capture and replay", "replay"):
        got_rep = S.read_report(bts.step(src))
        torch.cuda.synchronize()
        assert bts.graphs_captured == (0 if use == "eager first use" else 1)
        figs = {k: rel_err(torch.tensor(got_rep[k]), torch.tensor(rep[k])) for k in ("total_loss", "mwer_loss")}
        figs["dtheta"] = rel_err(ens.weight_logits.grad, want)
        print(use, {k: f"{v:.3g}" for k, v in figs.items()}, "dtheta", ens.weight_logits.grad.tolist())
        assert max(figs.values()) < TOL and got_rep["skipped"] is False, (use, figs)
        _compare(use, _grads(model), want_grads)


def test_captured_eval_step_follows_theta_without_recapture(fx):
    """One member takes nearly all the weight, then another whose decode differs: the captured
    step's ensemble hypotheses change with theta and equal a fresh EvalState on freeze()."""
    import scattennet_amd as S
    dev = _dev()
    src = _src(fx, dev)
    model = _build(fx, dev)
    heads = ("alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits")
    plain = S.EvalState(model, heads=heads, capacity=3, log_width=13)
    S.eval_step(model, src, plain)
    hyps = plain.hypotheses()
    keys = sorted(hyps[0])
    lists = {k: [h[k] for h in hyps] for k in keys}
    pairs = [(a, b) for a in keys for b in keys if a < b and lists[a] != lists[b]]
    print("decoded keys", keys, "pairs that decode differently", pairs)
    assert pairs  # the fixture's heads do not all decode alike
    of = {k.replace("gloss_logits", ""): k for k in heads}  # the log's names, as evaluate.logits_name gives them
    first, second = (heads.index(of[k]) for k in pairs[0])
    ens = S.LearnedEnsemble(heads).to(dev)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(32,), label_bucket=3, capacity=30,
                             heads=("fuse_coord_gloss_logits",), ensembles={ENS: ens})
    for _ in range(2):  # the eager first use, then the capture
        bes.step(src)
    assert bes.graphs_captured == 1
    seen = []
    for favoured in (first, second):
        theta = torch.full((5,), -10.0)
        theta[favoured] = 10.0
        ens.load_state_dict({"weight_logits": theta})
        before = len(bes.hypotheses())
        out = bes.step(src)  # a replay
        got = [h["learned_"] for h in bes.hypotheses()[before:]]
        fresh = S.EvalState(model, heads=("fuse_coord_gloss_logits",), capacity=3, log_width=13,
                            ensembles={ENS: ens.freeze()})
        want_out = S.eval_step(model, src, fresh)
        want = [h["learned_"] for h in fresh.hypotheses()]
        err = rel_err(out[ENS], want_out[ENS])
        print("weight on", heads[favoured], "->", got, "freeze():", want, "the head alone:", lists[pairs[0][len(seen)]],
              f"ensemble rel_err {err:.3e}")
        assert bes.graphs_captured == 1 and got == want and err < TOL
        seen.append(got)
    assert seen[0] != seen[1]
