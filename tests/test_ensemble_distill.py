"""Ensemble distillation, host side (scattennet_amd/distill.py; sca_distill_heads_fwd / _bwd of
include/scatten.h): the float64 restatement of tests/distill_ref.py against torch autograd through
the torch composition, the G = 1 identity, every argument error before any device call, and the
report layout with the new keys.  CPU only."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import heads_oracle as HO
from tests import distill_ref as DR
from tests import ensemble_ref as R

ALL = ("alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits")


def _torch_composition(students, members, student_weights, weights, mode, temp, start, lo=-100.0, hi=100.0):
    """What the grouped call replaces, in float64 with autograd: (losses, gradients)."""
    w = torch.tensor(R.normalised(weights, len(members)))
    lps = [torch.log_softmax(torch.from_numpy(x).double(), -1) for x in members]
    if mode == "prob":
        e = torch.logsumexp(torch.stack([lp + torch.log(w[g]) for g, lp in enumerate(lps)]), 0)
    else:
        e = torch.log_softmax(sum(w[g] * lp for g, lp in enumerate(lps)), -1)
    losses, grads = [], []
    for s, sw in zip(students, student_weights):
        x = torch.from_numpy(s).double().requires_grad_()
        C = x.shape[-1]
        kl = torch.nn.functional.kl_div(torch.log_softmax(x[..., start:] / temp, -1).reshape(-1, C - start),
                                        torch.softmax(e.detach()[..., start:] / temp, -1).reshape(-1, C - start),
                                        reduction="batchmean") * temp * temp
        loss = torch.clamp(sw * kl, lo, hi)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(x.grad.numpy())
    return np.array(losses), grads


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", DR.CASES, ids=DR.IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_torch_autograd_through_the_composition(case, mode):
    G, S, B, T, C, start, temp = case
    students, members = DR.case(G, S, B, T, C)
    sw = [1.0 + 0.5 * s for s in range(S)]
    for weights in (None, R.cycled_weights(G)):
        got_l, got_g = DR.distill(students, members, sw, weights, mode, temp, use_blank=start == 0)
        want_l, want_g = _torch_composition(students, members, sw, weights, mode, temp, start)
        assert float(np.abs(got_l - want_l).max()) <= 1e-12 * max(1.0, float(np.abs(want_l).max()))
        for a, b in zip(got_g, want_g):
            assert float(np.abs(a - b).max()) <= 1e-12 * max(1.0, float(np.abs(b).max()))
            assert (a[..., :start] == 0.0).all()


@pytest.mark.parametrize("case", DR.CASES[1:], ids=DR.IDS[1:])
@pytest.mark.parametrize("mode", R.MODES)
def test_parity_cases_keep_the_clamp_inactive_and_weight_1e4_closes_it(case, mode):
    """What the GPU file relies on: at weight 1 the losses of the N(0, 3) cases lie well inside
    the clamp; at weight 1e4 they are exactly hi = 100 with zero gradients."""
    G, S, B, T, C, start, temp = case
    students, members = DR.case(G, S, B, T, C)
    losses, _ = DR.distill(students, members, [1.0] * S, None, mode, temp, use_blank=start == 0)
    assert 0.5 < losses.min() and losses.max() < 50.0, losses
    losses, grads = DR.distill(students, members, [1e4] * S, None, mode, temp, use_blank=start == 0)
    assert (losses == 100.0).all() and all((g == 0.0).all() for g in grads)


def test_one_column_left_is_exactly_zero():
    G, S, B, T, C, start, temp = DR.CASES[0]
    students, members = DR.case(G, S, B, T, C)
    losses, grads = DR.distill(students, members, [1.0], None, "prob", temp)
    assert (losses == 0.0).all() and (grads[0] == 0.0).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_one_member_is_seqkd_on_its_logits(mode):
    """seqkd(s, ensemble([x])) == seqkd(s, x): the member's log-sum-exp cancels in the softmax."""
    students, members = DR.case(1, 2, 2, 5, 33)
    for s in students:
        a = HO.seqkd(s, R.ensemble(members, [2.5], mode), 1.5, 2.0, False, -100.0, 100.0)
        b = HO.seqkd(s, members[0], 1.5, 2.0, False, -100.0, 100.0)
        assert abs(a[0] - b[0]) <= 1e-13 * abs(b[0])
        assert float(np.abs(a[1] - b[1]).max()) <= 1e-15


def test_clamp_rows_stay_finite():
    students, members = DR.case(3, 2, 1, 4, 12, clamp_rows=True)
    for mode in R.MODES:
        losses, grads = DR.distill(students, members, [1.0, 1.0], None, mode)
        assert np.isfinite(losses).all() and all(np.isfinite(g).all() for g in grads)


# ------------------------------------------------------------------------ Python validation
def test_distill_errors():
    import scattennet_amd as S
    d = S.Distill("fuse_coord_gloss_logits", {"left": 1.0, "right": 0.0, "body": 2})
    assert d.students == ("left", "right", "body") and d.weights == (1.0, 0.0, 2.0) and d.T == 1.0
    spec = S.EnsembleSpec(ALL)
    assert S.Distill(spec, {"left": 1.0}, T=2).teacher is spec
    assert isinstance(S.Distill(S.LearnedEnsemble(ALL[:3]), {"left": 1.0}).teacher, S.LearnedEnsemble)
    assert S.check_distill(None, "x") is None and S.check_distill(d, "x") is d
    with pytest.raises(ValueError, match="unknown student"):
        S.Distill(spec, {"gloss_logits": 1.0})
    with pytest.raises(ValueError, match="distinct"):
        S.Distill(spec, [("left", 1.0), ("left", 2.0)])
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.Distill(spec, {f"k{i}": 1.0 for i in range(9)})
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.Distill(spec, {})
    for bad in (-1.0, float("nan"), float("inf"), "a", True, None):
        with pytest.raises(ValueError, match="weight"):
            S.Distill(spec, {"left": bad})
    for bad in (0, 0.0, -1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="temperature"):
            S.Distill(spec, {"left": 1.0}, T=bad)
    for bad in ("gloss_logits", None, 3, ("left", "right"), [spec]):
        with pytest.raises(ValueError, match="teacher"):
            S.Distill(bad, {"left": 1.0})
    with pytest.raises(ValueError, match="students"):
        S.Distill(spec, "left")
    with pytest.raises(ValueError, match="train_step: distill"):
        S.check_distill(spec, "train_step")
    with pytest.raises(ValueError, match="distill must be a Distill"):
        S.train_step(None, None, {}, distill=S.MWER(1.0))


def test_loss_validation_comes_before_the_device():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    f = S.ensemble_distillation_loss
    with pytest.raises(ValueError, match="between 1 and 8 students"):
        f([], [x], [])
    with pytest.raises(ValueError, match="between 1 and 8 students"):
        f([x] * 9, [x], [1.0] * 9)
    with pytest.raises(ValueError, match="between 1 and 8"):
        f([x], [x] * 9, [1.0])
    with pytest.raises(ValueError, match="same shape"):
        f([torch.randn(2, 8, 13)], [x], [1.0])
    with pytest.raises(ValueError, match="same shape"):
        f([x.double()], [x], [1.0])
    for bad in ([], [1.0, 2.0], [-1.0], [float("nan")], ["a"], 3.0):
        with pytest.raises(ValueError, match="student_weights"):
            f([x], [x, x], bad)
    with pytest.raises(ValueError, match="temperature"):
        f([x], [x], [1.0], T=0.0)
    with pytest.raises(ValueError, match="mode"):
        f([x], [x], [1.0], mode="mean")
    with pytest.raises(ValueError, match="weights"):
        f([x], [x, x], [1.0], weights=[1.0, 0.0])
    with pytest.raises(ValueError, match="not both"):
        f([x], [x, x], [1.0], weights=[1.0, 1.0], weight_logits=torch.zeros(2))
    with pytest.raises(ValueError, match="weight_logits"):
        f([x], [x, x], [1.0], weight_logits=torch.zeros(3))
    with pytest.raises(ValueError, match="clamp"):
        f([x], [x], [1.0], clamp=(1.0, -1.0))
    with pytest.raises(ValueError, match="use_blank"):
        f([x], [x], [1.0], use_blank=1)
    with pytest.raises(ValueError, match="more than one class"):
        f([torch.randn(2, 8, 1)], [torch.randn(2, 8, 1)], [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f([x], [x, x], [1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f([x.half()], [x.half()], [1.0])


# ------------------------------------------------------------------------ the C ABI's checks
def _abi():
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in ("sca_distill_heads_fwd", "sca_distill_heads_bwd", "sca_distill_heads_workspace_floats"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = L.EXPORTS[name]
    return L, lib


def test_c_argument_validation_makes_no_gpu_call():
    """Fake pointers throughout: a call that got past the checks would fault."""
    L, lib = _abi()
    hx, wx, sx, gx = L.DecodeHeads(), L.EnsembleWeights(), L.DistillStudents(), L.DistillGrads()
    for g in range(8):
        hx.logits[g] = 0x1000 + 0x100 * g
        wx.w[g] = 1.0
        sx.logits[g] = 0x2000 + 0x100 * g
        sx.weight[g] = 1.0
        gx.dlogits[g] = 0x3000 + 0x100 * g
    P = ctypes.c_void_p
    theta, vf, losses, ws, dl = P(0x4000), P(0x4100), P(0x5000), P(0x6000), P(0x7000)
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731

    def fwd(G=2, S=2, mode=0, B=2, T=3, C=5, start=1, temp=1.0, members=hx, weights=wx, theta=None, students=sx,
            valid=None, shift=0, losses=losses, ws=ws):
        return lib.sca_distill_heads_fwd(ref(members), G, ref(weights), theta, mode, ref(students), S, B, T, C, start,
                                         temp, -100.0, 100.0, valid, shift, losses, ws, None)

    def bwd(G=2, S=2, mode=0, B=2, T=3, C=5, start=1, temp=1.0, members=hx, weights=wx, theta=None, students=sx,
            valid=None, shift=0, dlosses=dl, ws=ws, grads=gx):
        return lib.sca_distill_heads_bwd(ref(members), G, ref(weights), theta, mode, ref(students), S, B, T, C, start,
                                         temp, valid, shift, dlosses, ws, ref(grads), None)

    hole, shole = L.DecodeHeads(), L.DistillStudents()
    hole.logits[0] = 0x1000
    shole.logits[0] = 0x2000
    for call in (fwd, bwd):
        # the ensemble entries' checks: the members, G, the weights, mode, the sizes
        assert call(G=0) == 1 and call(G=9) == 1 and call(mode=2) == 1 and call(mode=-1) == 1
        assert call(B=0) == 1 and call(T=0) == 1 and call(C=0) == 1
        assert call(members=None) == 1 and call(members=hole) == 1
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            w = L.EnsembleWeights()
            w.w[0], w.w[1] = 1.0, bad
            assert call(weights=w) == 1, bad
        # S, the students, temp, start
        assert call(S=0) == 1 and call(S=9) == 1
        assert call(students=None) == 1 and call(students=shole) == 1
        assert call(temp=0.0) == 1 and call(temp=-1.0) == 1 and call(temp=float("nan")) == 1
        assert call(start=-1) == 1 and call(start=5) == 1
        # the valid-frame arguments
        assert call(valid=vf, shift=-1) == 1 and call(valid=vf, shift=31) == 1
        # both or neither weight source
        assert call(theta=theta) == 1 and call(weights=None) == 1
        assert call(ws=None) == 1
    assert fwd(losses=None) == 1 and bwd(dlosses=None) == 1 and bwd(grads=None) == 1
    # an output that aliases an input or another output
    for p in (0x1000, 0x1100, 0x2000, 0x2100):  # a member, a student
        assert fwd(losses=P(p)) == 1 and fwd(ws=P(p)) == 1
    assert fwd(losses=ws) == 1
    assert fwd(weights=None, theta=theta, losses=theta) == 1 and fwd(weights=None, theta=theta, ws=theta) == 1
    assert fwd(valid=vf, losses=vf) == 1 and fwd(valid=vf, ws=vf) == 1
    for p in (0x1000, 0x1100, 0x2000, 0x2100, 0x6000, 0x7000, 0x3000):  # ..., ws, dlosses, another gradient
        g = L.DistillGrads()
        g.dlogits[0], g.dlogits[1] = 0x3000, p
        assert bwd(grads=g) == 1, hex(p)
    g = L.DistillGrads()
    g.dlogits[0] = 0x4000
    assert bwd(weights=None, theta=theta, grads=g) == 1
    # every entry null: nothing is launched
    assert bwd(grads=L.DistillGrads()) == 0
    with pytest.raises(ValueError, match="sca_distill_heads_fwd"):
        L.check(fwd(S=9), "sca_distill_heads_fwd")
    with pytest.raises(ValueError, match="sca_distill_heads_bwd"):
        L.check(bwd(G=9), "sca_distill_heads_bwd")


def test_workspace_size():
    _, lib = _abi()
    f = lib.sca_distill_heads_workspace_floats
    assert f(1, 1, 2, 3) == 5 * 6 + 1  # sca_seqkd's own layout
    assert f(3, 1, 2, 3) == 3 * (5 * 6 + 1)
    assert f(3, 5, 2, 3) == 3 * (5 * 6 + 1) + 2 * 3 * 6 * 5
    assert f(0, 1, 2, 3) == 0 and f(9, 1, 2, 3) == 0 and f(1, 0, 2, 3) == 0 and f(1, 9, 2, 3) == 0
    assert f(1, 1, 0, 3) == 0 and f(1, 1, 2, 0) == 0


# ------------------------------------------------------------------------------- the report
@pytest.mark.parametrize("students", [(), ("left", "right", "body")])
@pytest.mark.parametrize("with_mwer", [False, True])
def test_read_report_layout_with_the_new_keys(students, with_mwer):
    from scattennet_amd import model as M
    from scattennet_amd import train
    lay = M.report_layout(students)
    vals = torch.zeros(lay["words"], dtype=torch.float32)
    for i, k in enumerate(k for k in lay if k not in ("flags", "words")):
        vals[lay[k]] = 1.0 + i
    outputs = {f"{s}_distill_loss": None for s in students}
    outputs["finite_report"] = vals.view(torch.int32)
    plain = train.read_report(dict(outputs))
    assert "ensemble_kd_loss" not in plain and plain["skipped"] is False
    outputs["ensemble_kd_losses"] = torch.tensor([0.5, 0.25])
    outputs["ensemble_kd_loss"] = torch.tensor(0.75)
    outputs["ensemble_kd_report"] = torch.tensor([0.75])
    if with_mwer:
        outputs["mwer_report"] = torch.tensor([2.5, 0.125])
    rep = train.read_report(outputs)
    assert rep["ensemble_kd_loss"] == 0.75 and rep["skipped"] is False
    assert {k: v for k, v in rep.items() if k in plain} == plain  # the model's own terms, unmoved
    assert M._students_of(outputs) == list(students)  # no new key ends in _distill_loss
    if with_mwer:
        assert rep["mwer_loss"] == 2.5 and rep["mwer_risk"] == 0.125
    else:
        assert "mwer_loss" not in rep
    outputs["ensemble_kd_report"] = torch.tensor([float("nan")])
    assert train.read_report(outputs)["skipped"] is True
