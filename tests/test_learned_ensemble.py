"""The learned head ensemble, host side (scattennet_amd/ensemble.py: LearnedEnsemble,
ensemble_log_probs(weight_logits=...); sca_ensemble_log_probs_dw / _dw_bwd of include/scatten.h):
the float64 restatement of tests/ensemble_weight_ref.py against float64 torch autograd through the
composition with theta a leaf, the structural properties of d theta, every argument error before
any device call, and the entry points' declarations.  CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_grad_ref as GR
from tests import ensemble_ref as R
from tests import ensemble_weight_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (3, 2, 7, 70), (5, 2, 9, 33), (8, 1, 3, 1124), (2, 5, 53, 8)]  # (G, B, T, C)
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
CLAMPED = {(3, 2, 7, 70)}  # with the +-50 rows (ensemble_ref.case)
FWD, WSB, BWD = ("sca_ensemble_log_probs_dw", "sca_ensemble_log_probs_dw_workspace_bytes",
                 "sca_ensemble_log_probs_dw_bwd")


def _torch_composition(xs, theta, mode):
    """The composition the fused call replaces, on float64 tensors; theta may be a leaf."""
    lw = torch.log_softmax(theta, 0)
    lps = [torch.log_softmax(x, -1) for x in xs]
    if mode == "prob":
        return torch.logsumexp(torch.stack([lp + lw[g] for g, lp in enumerate(lps)]), 0)
    return torch.log_softmax(sum(torch.exp(lw[g]) * lp for g, lp in enumerate(lps)), -1)


def _autograd(xs, theta, mode, dout):
    ts = [torch.from_numpy(x).double().requires_grad_(True) for x in xs]
    th = torch.from_numpy(np.asarray(theta, np.float64)).requires_grad_(True)
    out = _torch_composition(ts, th, mode)
    out.backward(torch.from_numpy(dout).double())
    return out.detach().numpy(), [t.grad.numpy() for t in ts], th.grad.numpy()


def _err(got, want):
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_autograd_with_theta_a_leaf(shape, mode):
    G = shape[0]
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    dout = GR.dout_of(shape[1:])
    theta = WR.theta_of(G)
    want_out, want_dx, want_dt = _autograd(xs, theta, mode, dout)
    got_dx, got_dt = WR.vjp(xs, theta, mode, dout)
    figs = {"out": _err(WR.ensemble(xs, theta, mode), want_out), "dtheta": _err(got_dt, want_dt)}
    for g in range(G):
        figs[f"dx{g}"] = _err(got_dx[g], want_dx[g])
    print(mode, shape, {k: f"{v:.2e}" for k, v in figs.items()}, "max |dtheta|", float(np.abs(want_dt).max()))
    assert got_dt.shape == (G,) and np.isfinite(got_dt).all()
    assert max(figs.values()) <= 1e-12, figs
    if G >= 2:  # the GPU comparison against this reference is not vacuous
        assert float(np.abs(want_dt).max()) >= 1.0
    # theta = 0 is the equal-weights ensemble
    assert _err(WR.ensemble(xs, np.zeros(G), mode), R.ensemble(xs, None, mode)) <= 1e-15


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] >= 2], ids=[i for i, s in zip(IDS, SHAPES) if s[0] >= 2])
@pytest.mark.parametrize("mode", R.MODES)
def test_weight_gradients_sum_to_zero(shape, mode):
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    dt = WR.dtheta(xs, WR.theta_of(shape[0]), mode, GR.dout_of(shape[1:]))
    print(mode, shape, "sum", float(dt.sum()), "max", float(np.abs(dt).max()))
    assert abs(float(dt.sum())) <= 1e-12 * float(np.abs(dt).max())


@pytest.mark.parametrize("mode", R.MODES)
def test_rows_without_an_incoming_gradient_contribute_zero(mode):
    shape = (3, 2, 7, 70)
    xs = R.case(*shape, clamp_rows=True)
    theta = WR.theta_of(3)
    dout = GR.dout_of(shape[1:], zero_rows=5)
    part = WR.row_partials(xs, theta, mode, dout)
    assert part.shape == (14, 3) and (part[-5:] == 0).all() and np.abs(part[:-5]).max() > 0
    # so the members of those rows do not matter
    other = [x.copy() for x in xs]
    for x in other:
        x.reshape(-1, 70)[-5:] += 1.5
    assert np.array_equal(WR.row_partials(other, theta, mode, dout)[:-5], part[:-5])
    assert np.array_equal(WR.dtheta(other, theta, mode, dout), WR.dtheta(xs, theta, mode, dout))


def test_one_member_has_a_zero_weight_gradient():
    x = R.case(1, 2, 7, 70)
    dout = GR.dout_of((2, 7, 70))
    for mode in R.MODES:
        for theta in ([0.0], [2.5]):
            assert np.array_equal(WR.dtheta(x, theta, mode, dout), np.zeros(1))
            _, _, auto = _autograd(x, theta, mode, dout)
            assert abs(float(auto[0])) <= 1e-12


# ---------------------------------------------------------------------------- the entry points
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)


def test_entry_points_are_declared_exported_and_bound():
    from scattennet_amd import _lib
    src = _header()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, ret, count in ((FWD, "int", 9), (WSB, "long", 3), (BWD, "int", 13)):
        assert re.search(r"^\s*%s\s+%s\s*\(" % (ret, name), src, flags=re.M), name
        nargs = len(re.search(r"%s\s*\((.*?)\)" % name, src, flags=re.S).group(1).split(","))
        assert name in _lib.EXPORTS and len(_lib.EXPORTS[name][0]) == nargs == count, name
        assert hasattr(lib, name) and name in doc, name
    assert _lib.EXPORTS[WSB][1] is ctypes.c_long
    # the existing entries are as they were
    assert len(_lib.EXPORTS["sca_ensemble_log_probs"][0]) == 9
    assert len(_lib.EXPORTS["sca_ensemble_log_probs_bwd"][0]) == 11


def _bind(name):
    from scattennet_amd import _lib as L
    fn = getattr(ctypes.CDLL(L.LIB_PATH), name)
    fn.argtypes, fn.restype = L.EXPORTS[name]
    return fn


def test_workspace_bytes():
    fn = _bind(WSB)
    assert fn(2, 5, 53) == 4 * 2 * 265 and fn(8, 8, 64) == 4 * 8 * 512
    assert fn(1, 5, 53) == 0  # G = 1: d theta = 0, no partials
    assert fn(0, 5, 53) == 0 and fn(9, 5, 53) == 0 and fn(2, 0, 53) == 0 and fn(2, 5, 0) == 0
    assert fn(8, 65536, 65536) == 4 * 8 * 65536 * 65536  # no 32-bit overflow


THETA, OUT, DOUT, DTHETA, WS = 0x40000, 0x20000, 0x30000, 0x50000, 0x60000


def _tables():
    from scattennet_amd import _lib as L
    hx, gx = L.DecodeHeads(), L.EnsembleGrads()
    for g in range(8):
        hx.logits[g] = 0x1000 * (g + 1)
        gx.dlogits[g] = 0x100000 * (g + 1)
    return hx, gx


def _ref(s):
    return None if s is None else ctypes.byref(s)


def test_forward_argument_validation_makes_no_gpu_call():
    from scattennet_amd import _lib as L
    fn = _bind(FWD)
    hx, _ = _tables()

    def call(G=2, mode=0, B=2, T=3, C=5, heads=hx, theta=THETA, out=OUT):
        return fn(_ref(heads), G, theta, mode, B, T, C, out, None)
    assert call(G=0) == 1 and call(G=9) == 1 and call(mode=2) == 1 and call(mode=-1) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(C=0) == 1
    assert call(heads=None) == 1 and call(theta=None) == 1 and call(out=None) == 1
    assert call(out=THETA) == 1 and call(out=0x1000) == 1 and call(out=0x2000) == 1 and call(theta=0x2000) == 1
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000
    assert call(heads=hole) == 1
    with pytest.raises(ValueError, match=FWD):
        L.check(call(G=9), FWD)


def test_backward_argument_validation_makes_no_gpu_call():
    from scattennet_amd import _lib as L
    fn = _bind(BWD)
    hx, gx = _tables()

    def call(G=2, mode=0, B=2, T=3, C=5, heads=hx, theta=THETA, out=OUT, dout=DOUT, grads=gx, dtheta=DTHETA, ws=WS):
        return fn(_ref(heads), G, theta, mode, B, T, C, out, dout, _ref(grads), dtheta, ws, None)
    assert call(G=0) == 1 and call(G=9) == 1 and call(mode=2) == 1 and call(mode=-1) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(C=0) == 1
    assert call(heads=None) == 1 and call(theta=None) == 1 and call(grads=None) == 1
    assert call(out=None) == 1 and call(dout=None) == 1 and call(dout=OUT) == 1
    assert call(theta=OUT) == 1 and call(theta=DOUT) == 1 and call(theta=0x1000) == 1
    assert call(ws=None) == 1  # d theta is asked for with G >= 2
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000
    assert call(heads=hole) == 1
    # a gradient tensor that is out, dout, theta, a member (its own or another), another gradient
    # tensor, d theta or the workspace
    for alias in (OUT, DOUT, THETA, 0x1000, 0x2000, 0x200000, DTHETA, WS):
        g = L.EnsembleGrads()
        g.dlogits[0], g.dlogits[1] = alias, 0x200000
        assert call(grads=g) == 1, hex(alias)
    for alias in (OUT, DOUT, THETA, 0x1000, 0x2000, 0x100000, 0x200000):
        assert call(dtheta=alias) == 1, hex(alias)
        assert call(ws=alias) == 1, hex(alias)
    assert call(ws=DTHETA) == 1
    # nothing takes a gradient: the call returns without a launch; entries [G, 8) are ignored, and
    # neither the workspace nor its aliasing matters when d theta is not asked for
    none = L.EnsembleGrads()
    none.dlogits[2] = OUT
    assert call(grads=none, dtheta=None) == 0
    assert call(grads=none, dtheta=None, ws=None) == 0 and call(grads=none, dtheta=None, ws=OUT) == 0
    with pytest.raises(ValueError, match=BWD):
        L.check(call(G=9), BWD)


# ------------------------------------------------------------------------ Python validation
def test_weight_logits_argument_errors_before_any_device_call():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    good = torch.zeros(2)
    with pytest.raises(ValueError, match="not both"):
        S.ensemble_log_probs([x, x], [1.0, 2.0], weight_logits=good)
    for bad in ([0.0, 0.0], (0.0, 0.0), 0.0, "theta", np.zeros(2, np.float32)):
        with pytest.raises(ValueError, match="weight_logits must be a"):
            S.ensemble_log_probs([x, x], weight_logits=bad)
    for bad in (torch.zeros(3), torch.zeros(1), torch.zeros(2, 1), torch.zeros(()), torch.zeros(1, 2)):
        with pytest.raises(ValueError, match="shape"):
            S.ensemble_log_probs([x, x], weight_logits=bad)
    for bad in (torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.float64), torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
            S.ensemble_log_probs([x, x], weight_logits=bad)
    with pytest.raises(ValueError, match="device"):
        S.ensemble_log_probs([x, x], weight_logits=torch.zeros(2, device="meta"))
    with pytest.raises(ValueError, match="mode"):
        S.ensemble_log_probs([x, x], None, "mean", weight_logits=good)
    with pytest.raises(ValueError, match="differentiable"):
        S.ensemble_log_probs([x, x], weight_logits=good, differentiable=1)
    with pytest.raises(TypeError):
        S.ensemble_log_probs([x, x], None, "prob", good)  # keyword-only
    for dtype in (torch.float32, torch.float16, torch.bfloat16):  # valid: the call goes on to the device check
        for flag in (False, True):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                theta = torch.zeros(2, dtype=dtype, requires_grad=flag)
                S.ensemble_log_probs([x, x], weight_logits=theta, differentiable=flag)
    assert hasattr(S, "LearnedEnsembleLogProbsOp")


def test_learned_ensemble_is_a_module_with_one_parameter():
    import scattennet_amd as S
    ens = S.LearnedEnsemble(("left", "right", "body"))
    assert isinstance(ens, torch.nn.Module) and [n for n, _ in ens.named_parameters()] == ["weight_logits"]
    theta = ens.weight_logits
    assert theta.shape == (3,) and theta.dtype == torch.float32 and theta.requires_grad and bool((theta == 0).all())
    assert ens.members == ("left", "right", "body") and ens.mode == "prob"
    assert repr(ens) == "LearnedEnsemble(members=('left', 'right', 'body'), mode='prob')"
    assert ens.weights() == pytest.approx((1 / 3,) * 3, abs=1e-15)
    init = S.LearnedEnsemble(["left", "body"], "logprob", init=[1, 3])
    assert init.mode == "logprob"
    assert init.weight_logits.tolist() == pytest.approx([np.log(0.25), np.log(0.75)], abs=1e-7)
    assert init.weights() == pytest.approx((0.25, 0.75), abs=1e-7) and isinstance(init.weights(), tuple)
    frozen = init.freeze()
    assert type(frozen) is S.EnsembleSpec and frozen.members == ("left", "body") and frozen.mode == "logprob"
    assert frozen.weights == pytest.approx(init.weights(), abs=1e-15)
    # the state dict round trip, which is what a captured step follows without recapture
    other = S.LearnedEnsemble(["left", "body"], "logprob")
    other.load_state_dict(init.state_dict(), strict=True)
    assert torch.equal(other.weight_logits, init.weight_logits)
    # EnsembleSpec's validation of the members and the mode, and its weights' for init
    for members in ("left", (), ("left", "left"), ("left", "nose"), tuple("abcdefghi")):
        with pytest.raises(ValueError, match="EnsembleSpec"):
            S.LearnedEnsemble(members)
    with pytest.raises(ValueError, match="mode"):
        S.LearnedEnsemble(("left", "right"), "mean")
    for bad in ([1.0], [1.0, 2.0, 3.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")], "ab", 3.0):
        with pytest.raises(ValueError, match="LearnedEnsemble"):
            S.LearnedEnsemble(("left", "right"), init=bad)


def test_learned_ensemble_compute_passes_the_parameter_on(monkeypatch):
    import scattennet_amd as S
    from scattennet_amd import ensemble as E
    seen = []

    def fake(xs, weights=None, mode="prob", *, weight_logits=None, differentiable=False):
        seen.append((list(xs), weights, mode, weight_logits, differentiable))
        return "e"
    monkeypatch.setattr(E, "ensemble_log_probs", fake)
    ens = S.LearnedEnsemble(("left", "body"), mode="logprob")
    outputs = {"left": 1, "right": 2, "body": 3}
    assert ens.compute(outputs) == "e" and ens.compute(outputs, differentiable=True) == "e"
    assert seen[0][:3] == ([1, 3], None, "logprob") and seen[0][3] is ens.weight_logits and seen[0][4] is False
    assert seen[1][3] is ens.weight_logits and seen[1][4] is True


def test_check_ensembles_takes_a_learned_ensemble():
    import scattennet_amd as S
    from scattennet_amd.ensemble import check_ensembles
    ens, spec = S.LearnedEnsemble(("left", "right")), S.EnsembleSpec(("left", "body"))
    got = check_ensembles(("fuse_coord_gloss_logits",), {"learned_gloss_logits": ens, "fixed_gloss_logits": spec}, "t")
    assert list(got) == ["learned_gloss_logits", "fixed_gloss_logits"] and got["learned_gloss_logits"] is ens
    for bad in (torch.nn.Linear(2, 2), ens.weight_logits, ("left", "right"), None, "left"):
        with pytest.raises(ValueError, match="EnsembleSpec or a LearnedEnsemble"):
            check_ensembles(("fuse_coord_gloss_logits",), {"x_gloss_logits": bad}, "t")
    with pytest.raises(ValueError, match="gloss_logits"):
        check_ensembles(("left",), {"learned": ens}, "t")
    with pytest.raises(ValueError, match="more than"):
        check_ensembles(("left",) * 7, {"a_gloss_logits": ens, "b_gloss_logits": spec}, "t")


def test_mwer_takes_a_learned_ensemble_as_a_head():
    import scattennet_amd as S
    ens = S.LearnedEnsemble(("left", "right", "body"), mode="logprob")
    m = S.MWER(0.5, 4, 3, reference=True, head=ens)
    assert m.head is ens and m.heads == (ens,)
    assert "LearnedEnsemble(members=('left', 'right', 'body'), mode='logprob')" in repr(m)
    spec, other = S.EnsembleSpec(("left", "body")), S.LearnedEnsemble(("left", "right", "body"), mode="logprob")
    mixed = S.MWER(0.5, head=("fuse_coord_gloss_logits", ens, spec, other))
    assert mixed.heads == ("fuse_coord_gloss_logits", ens, spec, other)
    with pytest.raises(ValueError, match="distinct"):
        S.MWER(0.5, head=(ens, ens))
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.MWER(0.5, head=tuple(S.LearnedEnsemble(("left",)) for _ in range(9)))
    for bad in (torch.nn.Linear(2, 2), ens.weight_logits):
        with pytest.raises(ValueError, match="head"):
            S.MWER(0.5, head=(ens, bad))


def test_the_steps_clear_the_learned_ensembles_gradients_with_the_models():
    import scattennet_amd as S
    from scattennet_amd.train import step_parameters
    model = torch.nn.Linear(3, 2)
    ens, other = S.LearnedEnsemble(("left", "right")), S.LearnedEnsemble(("left", "body"))
    spec = S.EnsembleSpec(("left", "body"))
    ids = lambda ps: [id(p) for p in ps]  # noqa: E731
    own = ids(model.parameters())
    assert ids(step_parameters(model, None)) == own
    assert ids(step_parameters(model, S.MWER(0.5))) == own
    assert ids(step_parameters(model, S.MWER(0.5, head=spec))) == own
    assert ids(step_parameters(model, S.MWER(0.5, head=ens))) == own + [id(ens.weight_logits)]
    mixed = S.MWER(0.5, head=("left", ens, spec, other))
    assert ids(step_parameters(model, mixed)) == own + [id(ens.weight_logits), id(other.weight_logits)]
    # the module is not part of the model: its checkpoint keys are its own
    assert list(ens.state_dict()) == ["weight_logits"]
