"""Ensemble distillation on the GPU (sca_distill_heads_fwd / _bwd, scattennet_amd/distill.py):
the grouped call against the float64 restatement of tests/distill_ref.py and against the GPU
composition it replaces, the clamp gate, the bitwise G = 1 identity with `distillation_loss`,
valid frames, null and zero entries, capture, and the steps with `distill=`.

The bound is the project's relative one (TOL of tests/test_gpu_ensemble.py: max abs error over
max abs reference).  Measured figures are printed before they are asserted."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import distill_ref as DR
from tests import ensemble_ref as R
from tests.golden_util import close, rel_err
from tests.mwer_gpu import fx  # noqa: F401  (the fixture, by name)
from tests.mwer_gpu import ADAM, TOL, _bits, _dev, _grads

pytestmark = pytest.mark.gpu

MEMBERS = ("left", "right", "body", "fuse_coord_gloss_logits")
STUDENTS = {"left": 1.0, "right": 0.5, "body": 0.25}


def _t(arrays, dev, grad=False):
    return [torch.from_numpy(a).to(dev).requires_grad_(grad) for a in arrays]


def _call(students, members, sw, dev, dlosses=None, **kw):
    """The grouped call on host arrays: (losses, gradients) on the device."""
    import scattennet_amd as S
    sd, md = _t(students, dev, grad=True), _t(members, dev)
    losses = S.ensemble_distillation_loss(sd, md, sw, **kw)
    dl = torch.ones_like(losses) if dlosses is None else torch.tensor(dlosses, device=dev)
    losses.backward(dl)
    torch.cuda.synchronize()
    return losses.detach(), [s.grad for s in sd]


@functools.lru_cache(maxsize=None)
def _ref(case, mode, weight=1.0, weighted=False):
    G, S, B, T, C, start, temp = case
    students, members = DR.case(G, S, B, T, C)
    w = R.cycled_weights(G) if weighted else None
    return DR.distill(students, members, [weight] * S, w, mode, temp, use_blank=start == 0)


def _figs(losses, grads, want_l, want_g):
    figs = {"loss": rel_err(losses, torch.from_numpy(want_l))}
    for s, (g, w) in enumerate(zip(grads, want_g)):
        figs[f"ds{s}"] = rel_err(g, torch.from_numpy(w))
    return figs


# ------------------------------------------------------------------ parity with the restatement
@pytest.mark.parametrize("case", DR.CASES, ids=DR.IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_losses_and_gradients_against_the_restatement(case, mode):
    G, S, B, T, C, start, temp = case
    dev = _dev()
    students, members = DR.case(G, S, B, T, C)
    want_l, want_g = _ref(case, mode)
    losses, grads = _call(students, members, [1.0] * S, dev, mode=mode, T=temp, use_blank=start == 0)
    if case == DR.CASES[0]:  # one column left
        print(case, mode, "losses", losses.tolist(), "max |grad|", float(grads[0].abs().max()))
        assert (want_l == 0.0).all() and bool((losses == 0).all()) and bool((grads[0] == 0).all())
        return
    figs = _figs(losses, grads, want_l, want_g)
    print(case, mode, {k: f"{v:.3g}" for k, v in figs.items()}, "losses", want_l.tolist())
    assert 0.5 < want_l.min() and want_l.max() < 50.0  # the clamp is inactive
    assert all(bool((g[..., :start] == 0).all()) for g in grads)
    assert max(figs.values()) < TOL, figs


@pytest.mark.parametrize("mode", R.MODES)
def test_rows_at_the_heads_clamp_stay_finite(mode):
    """ensemble_ref.case(..., clamp_rows=True): members at +-50 against each other and a row that is
    one-hot but for rounding.  At this shape the restatement gives 6.11 / 6.14 ("prob") and
    5.42 / 5.58 ("logprob"); measured error at most 1.9e-7."""
    dev = _dev()
    students, members = DR.case(3, 2, 2, 4, 260, clamp_rows=True)
    want_l, want_g = DR.distill(students, members, [1.0, 1.0], None, mode)
    losses, grads = _call(students, members, [1.0, 1.0], dev, mode=mode)
    figs = _figs(losses, grads, want_l, want_g)
    print(mode, {k: f"{v:.3g}" for k, v in figs.items()}, "losses", want_l.tolist())
    assert bool(torch.isfinite(losses).all()) and all(bool(torch.isfinite(g).all()) for g in grads)
    assert max(figs.values()) < TOL, figs


@pytest.mark.parametrize("mode", R.MODES)
def test_host_weights_device_scores_and_a_student_that_is_a_member(mode):
    import scattennet_amd as S
    dev = _dev()
    case = DR.CASES[2]
    G, Sn, B, T, C, start, temp = case
    students, members = DR.case(G, Sn, B, T, C)
    w = R.cycled_weights(G)
    want_l, want_g = _ref(case, mode, weighted=True)
    # non-uniform host weights
    losses, grads = _call(students, members, [1.0] * Sn, dev, mode=mode, T=temp, weights=w)
    figs = _figs(losses, grads, want_l, want_g)
    print(mode, "host weights", {k: f"{v:.3g}" for k, v in figs.items()})
    assert max(figs.values()) < TOL, figs
    # the same weights as device scores: theta = log w
    theta = torch.tensor(np.log(R.normalised(w, G)), dtype=torch.float32, device=dev).requires_grad_(True)
    losses, grads = _call(students, members, [1.0] * Sn, dev, mode=mode, T=temp, weight_logits=theta)
    figs = _figs(losses, grads, want_l, want_g)
    print(mode, "device scores", {k: f"{v:.3g}" for k, v in figs.items()})
    assert max(figs.values()) < TOL and theta.grad is None, figs  # the teacher is detached
    # co-distillation: student 0 is member 1, as one tensor
    md = _t(members, dev, grad=True)
    sd = [md[1]] + _t(students[1:], dev, grad=True)
    want_l, want_g = DR.distill([members[1]] + students[1:], members, [1.0] * Sn, w, mode, temp)
    losses = S.ensemble_distillation_loss(sd, md, [1.0] * Sn, weights=w, mode=mode, T=temp)
    losses.sum().backward()
    figs = _figs(losses, [s.grad for s in sd], want_l, want_g)
    print(mode, "student 0 is member 1", {k: f"{v:.3g}" for k, v in figs.items()})
    assert max(figs.values()) < TOL and md[0].grad is None and md[2].grad is None, figs


# ------------------------------------------------------------------ the clamp gate
@pytest.mark.parametrize("case", DR.CASES[1:], ids=DR.IDS[1:])
@pytest.mark.parametrize("mode", R.MODES)
def test_weight_1e4_closes_the_clamp_gate(case, mode):
    G, S, B, T, C, start, temp = case
    dev = _dev()
    students, members = DR.case(G, S, B, T, C)
    want_l, want_g = _ref(case, mode, weight=1e4)
    assert (want_l == 100.0).all() and all((g == 0.0).all() for g in want_g)
    losses, grads = _call(students, members, [1e4] * S, dev, mode=mode, T=temp, use_blank=start == 0)
    print(case, mode, "losses", losses.tolist(), "max |grad|", max(float(g.abs().max()) for g in grads))
    assert bool((losses == 100.0).all()) and all(bool((g == 0).all()) for g in grads)


# ------------------------------------------------------------------ G = 1: bitwise the single call
@pytest.mark.parametrize("valid", [False, True], ids=["plain", "valid"])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 8, 260), (2, 8, 1124)], ids=lambda s: "B%d_T%d_C%d" % s)
def test_one_member_is_bitwise_distillation_loss_per_student(shape, valid):
    import scattennet_amd as S
    dev = _dev()
    B, T, C = shape
    students, members = DR.case(1, 3, B, T, C)
    sw, temp = [1.0, 0.5, 0.25], 2.0
    v = (torch.tensor([5 << 1], dtype=torch.int32, device=dev), 1) if valid else None
    dl = [1.0, -0.5, 2.0]
    losses, grads = _call(students, members, sw, dev, dlosses=dl, T=temp, valid=v)
    q = _t(members, dev)[0]
    for s in range(3):
        x = _t(students[s:s + 1], dev, grad=True)[0]
        one = S.distillation_loss(x, q, sw[s], T=temp, valid=v)
        one.backward(torch.tensor(dl[s], device=dev))
        assert torch.equal(_bits(one), _bits(losses[s])), (s, float(one), float(losses[s]))
        assert torch.equal(_bits(x.grad), _bits(grads[s])), s
        assert float(x.grad.abs().max()) > 0
    print(shape, "valid" if valid else "plain", "bitwise the", 3, "single calls; losses", losses.tolist())


# ------------------------------------------------------------------ the GPU composition
@pytest.mark.parametrize("case", DR.CASES[1:], ids=DR.IDS[1:])
@pytest.mark.parametrize("mode", R.MODES)
def test_against_the_gpu_composition(case, mode):
    import scattennet_amd as S
    from scattennet_amd.heads import SeqKDOp
    G, Sn, B, T, C, start, temp = case
    dev = _dev()
    students, members = DR.case(G, Sn, B, T, C)
    w = R.cycled_weights(G)
    losses, grads = _call(students, members, [1.0] * Sn, dev, mode=mode, T=temp, weights=w, use_blank=start == 0)
    e = S.ensemble_log_probs(_t(members, dev), w, mode)
    for s in range(Sn):
        x = _t(students[s:s + 1], dev, grad=True)[0]
        # distillation_loss, with the case's own first column (it has use_blank=False built in)
        one = SeqKDOp.apply(x, e.detach(), start, float(temp), 1.0, -100.0, 100.0)
        one.backward()
        figs = {"loss": rel_err(losses[s], one), "ds": rel_err(grads[s], x.grad)}
        print(case, mode, "student", s, {k: f"{v:.3g}" for k, v in figs.items()})
        assert max(figs.values()) < TOL, figs


# ------------------------------------------------------------------ valid frames
@pytest.mark.parametrize("G", [1, 3])
def test_valid_frames_equal_the_unpadded_call_and_pad_with_exact_zeros(G):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, nv, Sn = 2, 8, 260, 5, 2
    students, members = DR.case(G, Sn, B, T, C)
    sw = [1.0, 0.5]
    vf = torch.tensor([nv], dtype=torch.int32, device=dev)
    kw = dict(mode="logprob", weights=R.cycled_weights(G))
    losses, grads = _call(students, members, sw, dev, valid=(vf, 0), **kw)
    want_l, want_g = _call([s[:, :nv].copy() for s in students], [m[:, :nv].copy() for m in members], sw, dev, **kw)
    figs = {"loss": rel_err(losses, want_l)}
    for s in range(Sn):
        figs[f"ds{s}"] = rel_err(grads[s][:, :nv], want_g[s])
        assert bool((grads[s][:, nv:] == 0).all()) and float(grads[s][:, :nv].abs().max()) > 0
    print("G", G, {k: f"{v:.3g}" for k, v in figs.items()})
    assert max(figs.values()) < TOL, figs
    # a capture follows the scalar
    sd, md = _t(students, dev, grad=True), _t(members, dev)

    def chain():
        for s in sd:
            s.grad = None
        out = S.ensemble_distillation_loss(sd, md, sw, valid=(vf, 0), **kw)
        out.sum().backward()
        return [out.detach()] + [s.grad for s in sd]

    graph, outs = _capture(chain)
    for n in (3, 8, 5):
        vf.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (n, i)
        assert all(bool((g[:, n:] == 0).all()) and float(g[:, n - 1].abs().max()) > 0 for g in got[1:])
    assert torch.equal(_bits(got[0]), _bits(losses))


def _capture(chain):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    return graph, outs


# ------------------------------------------------------------------ null and zero entries
@pytest.mark.parametrize("G", [1, 3])
def test_null_and_zero_entries(G):
    import scattennet_amd as S
    from scattennet_amd import _lib as L
    dev = _dev()
    Sn, B, T, C = 3, 2, 4, 260
    students, members = DR.case(G, Sn, B, T, C)
    sd, md = _t(students, dev), _t(members, dev)
    sd[0].requires_grad_(True)
    sd[2].requires_grad_(True)
    losses = S.ensemble_distillation_loss(sd, md, [1.0] * Sn)
    losses.backward(torch.tensor([1.0, 1.0, 0.0], device=dev))
    assert sd[1].grad is None and float(sd[0].grad.abs().max()) > 0
    assert bool((sd[2].grad == 0).all())  # dloss_s = 0
    # the C entry with a null middle entry: the buffer beside it is untouched
    lib = L.lib()
    ws = torch.empty(lib.sca_distill_heads_workspace_floats(Sn, G, B, T), device=dev)
    out, dl = torch.empty(Sn, device=dev), torch.ones(Sn, device=dev)
    buf = torch.full((3, B, T, C), 7.5, device=dev)
    hx, wx, sx, gx = L.decode_heads(md), L.EnsembleWeights(), L.DistillStudents(), L.DistillGrads()
    for g in range(G):
        wx.w[g] = 1.0 / G  # what the Python call hands over for weights=None
    for s in range(Sn):
        sx.logits[s], sx.weight[s] = sd[s].data_ptr(), 1.0
    gx.dlogits[0], gx.dlogits[2] = buf[0].data_ptr(), buf[2].data_ptr()
    args = (ctypes.byref(hx), G, ctypes.byref(wx), None, 0, ctypes.byref(sx), Sn, B, T, C, 1, 1.0)
    L.check(lib.sca_distill_heads_fwd(*args, -100.0, 100.0, None, 0, L.ptr(out), L.ptr(ws), L.stream_handle()), "fwd")
    L.check(lib.sca_distill_heads_bwd(*args, None, 0, L.ptr(dl), L.ptr(ws), ctypes.byref(gx), L.stream_handle()), "bwd")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(losses.detach()))
    assert bool((buf[1] == 7.5).all()) and torch.equal(_bits(buf[0]), _bits(sd[0].grad))
    assert float(buf[2].abs().max()) > 0 and not bool((buf[2] == 7.5).any())


# ------------------------------------------------------------------ capture
@pytest.mark.parametrize("learned", [False, True], ids=["host_weights", "theta"])
def test_captured_call_replays_bitwise(learned):
    import scattennet_amd as S
    dev = _dev()
    G, Sn, B, T, C = 3, 2, 2, 7, 260
    students, members = DR.case(G, Sn, B, T, C, clamp_rows=True)
    sd, md = _t(students, dev, grad=True), _t(members, dev)
    theta = torch.tensor([0.3, -0.2, 0.1], device=dev)
    kw = {"weight_logits": theta} if learned else {"weights": R.cycled_weights(G)}
    dl = torch.tensor([1.0, -0.5], device=dev)

    def chain():
        res = []
        for mode in R.MODES:
            for s in sd:
                s.grad = None
            out = S.ensemble_distillation_loss(sd, md, [1.0, 0.5], mode=mode, T=2.0, **kw)
            out.backward(dl)
            res += [out.detach()] + [s.grad for s in sd]
        return res

    graph, outs = _capture(chain)
    first = None
    for seed in (None, 5, "theta"):  # the captured inputs, refilled ones, then a changed theta
        if seed == "theta":
            if not learned:
                continue
            theta.copy_(torch.tensor([-1.0, 0.5, 2.0], device=dev))
        elif seed is not None:
            new_s, new_m = DR.case(G, Sn, B, T, C, seed=seed)
            with torch.no_grad():
                for x, new in zip(sd + md, new_s + new_m):
                    x.copy_(torch.from_numpy(new))
                dl.mul_(-0.5)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)
        assert all(float(t.abs().max()) > 0 for t in got)
        if seed == "theta":
            assert not torch.equal(first[0], got[0])  # the replay read the new theta
        first = got
        print("replay with", seed, "bitwise the eager chain")


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_reduced_precision_logits_take_the_fp32_path(dtype):
    import scattennet_amd as S
    dev = _dev()
    students, members = DR.case(3, 2, 2, 4, 260)
    low_s = [x.to(dtype).requires_grad_(True) for x in _t(students, dev)]
    low_m = [x.to(dtype) for x in _t(members, dev)]
    losses = S.ensemble_distillation_loss(low_s, low_m, [1.0, 0.5])
    losses.sum().backward()
    s32 = [x.detach().float().requires_grad_(True) for x in low_s]
    want = S.ensemble_distillation_loss(s32, [x.float() for x in low_m], [1.0, 0.5])
    want.sum().backward()
    assert losses.dtype == dtype and torch.equal(losses, want.to(dtype))
    for a, b in zip(low_s, s32):
        assert a.grad.dtype == dtype and torch.equal(a.grad, b.grad.to(dtype))


# ------------------------------------------------------------------ the steps
def _build(fx, dev, self_distillation=True):
    import scattennet_amd as S
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    cfg["self_distillation"] = self_distillation
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


def _trainer(fx, dev, self_distillation=True, **adam):
    import scattennet_amd as S
    model = _build(fx, dev, self_distillation)
    return model, S.FusedAdam(model.parameters(), **{**ADAM, **adam})


def _distill(mode="prob"):
    import scattennet_amd as S
    return S.Distill(S.EnsembleSpec(MEMBERS, weights=[1, 2, 3, 4], mode=mode), STUDENTS, T=2.0)


def _by_hand(fx, src, mode, self_distillation):
    """The step composed from the public calls on a twin model: (kd losses, gradients)."""
    import scattennet_amd as S
    model = _build(fx, _dev(), self_distillation)
    out = model(src)
    e = S.ensemble_log_probs([out[k] for k in MEMBERS], [1, 2, 3, 4], mode)
    kd = torch.stack([S.distillation_loss(out[k], e, w, T=2.0) for k, w in STUDENTS.items()])
    (out["total_loss"] + kd.sum()).backward()
    torch.cuda.synchronize()
    return kd.detach(), _grads(model)


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


@pytest.mark.parametrize("self_distillation", [True, False], ids=["with_self_distillation", "instead_of_it"])
@pytest.mark.parametrize("mode", R.MODES)
def test_train_step_with_distill_equals_the_step_composed_by_hand(fx, mode, self_distillation):
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev, self_distillation)
    out = S.train_step(model, opt, src, distill=_distill(mode))
    rep = S.read_report(out)
    torch.cuda.synchronize()
    want_kd, want = _by_hand(fx, src, mode, self_distillation)
    print(mode, self_distillation, "ensemble_kd_losses", out["ensemble_kd_losses"].tolist(), "by hand", want_kd.tolist())
    assert out["ensemble_kd_losses"].shape == (3,) and rep["skipped"] is False
    assert rel_err(out["ensemble_kd_losses"], want_kd) < TOL and float(want_kd.min()) > 0
    assert rep["ensemble_kd_loss"] == float(out["ensemble_kd_loss"].detach()) and "mwer_loss" not in rep
    assert ("left_distill_loss" in rep) is self_distillation
    assert not [k for k in set(out) - set(model(src)) if k.endswith("_distill_loss")]
    grads = _grads(model)
    _compare(f"{mode} {self_distillation}", grads, want)
    for k in ("left", "right", "body"):  # the classifiers of the students take the term's gradient
        assert float(grads[f"recognition_head.{k}_gloss_classifier.weight"].abs().max()) > 0


def test_read_report_is_one_copy_also_with_mwer(fx, monkeypatch):
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev)
    out = S.train_step(model, opt, src, mwer=S.MWER(0.5, 3, 2), distill=_distill())
    torch.cuda.synchronize()
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (copies.append(t.device.type), real(t, *a, **k))[1])
    rep = S.read_report(out)
    monkeypatch.undo()
    assert copies.count("cuda") == 1, copies
    assert rep["ensemble_kd_loss"] == float(out["ensemble_kd_loss"].detach())
    assert rep["mwer_loss"] == float(out["mwer_loss"].detach())
    assert abs(rep["mwer_risk"] - float(out["mwer_risk"].mean())) < 1e-6 and rep["skipped"] is False


def test_a_nan_in_a_students_logits_skips_the_update(fx):
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev, lr=1e-2)
    with torch.no_grad():
        model.recognition_head.left_gloss_classifier.bias[1] = float("nan")
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    out = S.train_step(model, opt, src, distill=_distill())
    torch.cuda.synchronize()
    assert int(opt.skipped) == 1
    for k, p in model.named_parameters():
        assert torch.equal(_bits(p.detach()), _bits(before[k])), k
    with pytest.raises(ValueError, match="left"):
        S.read_report(out)
    # the guard of the term itself: a non-finite ensemble_kd_loss gives a NaN guard
    guard = torch.tensor(1.25, device=dev)
    assert torch.isnan(S.mwer_guard(guard, torch.tensor(float("inf"), device=dev)))


def test_bucketed_step_with_distill_equals_the_eager_unpadded_step(fx):
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    eager_model, eager_opt = _trainer(fx, dev)
    eager_out = S.train_step(eager_model, eager_opt, src, distill=_distill())
    rep = S.read_report(eager_out)
    torch.cuda.synchronize()
    want = _grads(eager_model)
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3, distill=_distill())
    for use in ("eager first use", "capture and replay", "replay"):
        got = bts.step(src)
        got_rep = S.read_report(got)
        torch.cuda.synchronize()
        assert bts.graphs_captured == (0 if use == "eager first use" else 1)
        figs = {k: rel_err(torch.tensor(got_rep[k]), torch.tensor(rep[k])) for k in ("total_loss", "ensemble_kd_loss")}
        figs["ensemble_kd_losses"] = rel_err(got["ensemble_kd_losses"], eager_out["ensemble_kd_losses"])
        print(use, {k: f"{v:.3g}" for k, v in figs.items()})
        _compare(use, _grads(model), want)
        assert max(figs.values()) < TOL and got_rep["skipped"] is False, (use, figs)
