"""The differentiable head ensemble, host side (scattennet_amd/ensemble.py, mwer.py;
sca_ensemble_log_probs_bwd of include/scatten.h): the float64 restatement of
tests/ensemble_grad_ref.py against float64 torch autograd through the composition the fused call
replaces, every argument error before any device call, and the entry point's declaration.
CPU only."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_grad_ref as GR
from tests import ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1, 2), (2, 3, 5, 6), (3, 2, 7, 70), (5, 2, 9, 33), (8, 1, 3, 1124)]  # (G, B, T, C)
IDS = ["G%d_B%d_T%d_C%d" % s for s in SHAPES]
CLAMPED = {(3, 2, 7, 70)}  # with the +-50 rows (ensemble_ref.case)
NAME = "sca_ensemble_log_probs_bwd"


def _torch_composition(xs, weights, mode):
    """tests/test_ensemble.py's composition, on float64 tensors that may require a gradient."""
    w = torch.tensor(R.normalised(weights, len(xs)))
    lps = [torch.log_softmax(x, -1) for x in xs]
    if mode == "prob":
        return torch.logsumexp(torch.stack([lp + torch.log(w[g]) for g, lp in enumerate(lps)]), 0)
    return torch.log_softmax(sum(w[g] * lp for g, lp in enumerate(lps)), -1)


def _autograd(xs, weights, mode, dout):
    ts = [torch.from_numpy(x).double().requires_grad_(True) for x in xs]
    _torch_composition(ts, weights, mode).backward(torch.from_numpy(dout).double())
    return [t.grad.numpy() for t in ts]


# -------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("mode", R.MODES)
def test_restatement_equals_autograd_through_the_torch_composition(shape, mode):
    G = shape[0]
    xs = R.case(*shape, clamp_rows=shape in CLAMPED)
    dout = GR.dout_of(shape[1:])
    for weights in (None, R.cycled_weights(G)):
        got = GR.vjp(xs, weights, mode, dout)
        want = _autograd(xs, weights, mode, dout)
        assert len(got) == G
        for g in range(G):
            assert got[g].shape == xs[g].shape and np.isfinite(got[g]).all()
            err = float(np.abs(got[g] - want[g]).max()) / max(1.0, float(np.abs(want[g]).max()))
            assert err <= 1e-12, (mode, weights, g, err)


@pytest.mark.parametrize("mode", R.MODES)
def test_rows_without_an_incoming_gradient_have_zero_gradients(mode):
    shape = (3, 2, 7, 70)
    xs = R.case(*shape, clamp_rows=True)
    dout = GR.dout_of(shape[1:], zero_rows=5)
    for dx in GR.vjp(xs, R.cycled_weights(3), mode, dout):
        rows = dx.reshape(-1, shape[-1])
        assert (rows[-5:] == 0).all() and np.abs(rows[:-5]).max() > 0
    # the all-zero row among the clamp rows too
    dout = GR.dout_of(shape[1:])
    dout.reshape(-1, shape[-1])[:3] = 0.0
    for dx in GR.vjp(xs, None, mode, dout):
        assert (dx.reshape(-1, shape[-1])[:3] == 0).all()


def test_member_gradients_sum_to_the_log_softmax_backward_of_the_mean_for_one_member():
    """G = 1: both modes are log_softmax, whose backward is dout - softmax sum dout."""
    x = R.case(1, 2, 7, 70)
    dout = GR.dout_of((2, 7, 70))
    want = dout - np.exp(R.log_softmax(x[0])) * dout.astype(np.float64).sum(-1, keepdims=True)
    for mode in R.MODES:
        assert float(np.abs(GR.vjp(x, [2.5], mode, dout)[0] - want).max()) <= 1e-12


# ---------------------------------------------------------------------------- the entry point
def test_entry_point_is_declared_exported_and_bound():
    from scattennet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)
    assert re.search(r"^\s*int\s+%s\s*\(" % NAME, src, flags=re.M)
    assert NAME in _lib.EXPORTS
    nargs = len(re.search(r"%s\s*\((.*?)\)" % NAME, src, flags=re.S).group(1).split(","))
    assert len(_lib.EXPORTS[NAME][0]) == nargs == 11
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert ctypes.sizeof(_lib.EnsembleGrads) == ctypes.sizeof(ctypes.c_void_p) * _lib.EVAL_MAX_HEADS
    assert "sca_ensemble_grads" in src
    assert NAME in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the forward's entry is as it was
    assert len(_lib.EXPORTS["sca_ensemble_log_probs"][0]) == 9


def test_c_argument_validation_makes_no_gpu_call():
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    fn = getattr(lib, NAME)
    fn.argtypes, fn.restype = L.EXPORTS[NAME]
    hx, wx, gx = L.DecodeHeads(), L.EnsembleWeights(), L.EnsembleGrads()
    for g in range(8):
        hx.logits[g] = 0x1000 * (g + 1)
        wx.w[g] = 1.0
        gx.dlogits[g] = 0x100000 * (g + 1)
    out, dout = ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)

    def call(G=2, mode=0, B=2, T=3, C=5, heads=hx, weights=wx, out=out, dout=dout, grads=gx):
        ref = lambda s: None if s is None else ctypes.byref(s)  # noqa: E731
        return fn(ref(heads), G, ref(weights), mode, B, T, C, out, dout, ref(grads), None)
    assert call(G=0) == 1 and call(G=9) == 1 and call(mode=2) == 1 and call(mode=-1) == 1
    assert call(B=0) == 1 and call(T=0) == 1 and call(C=0) == 1
    assert call(heads=None) == 1 and call(weights=None) == 1 and call(grads=None) == 1
    assert call(out=None) == 1 and call(dout=None) == 1 and call(dout=out) == 1
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000
    assert call(heads=hole) == 1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        w = L.EnsembleWeights()
        w.w[0], w.w[1] = 1.0, bad
        assert call(weights=w) == 1, bad
    # a gradient tensor that is out, dout, a member (its own or another) or another gradient tensor
    for alias in (0x20000, 0x30000, 0x1000, 0x2000, 0x200000):
        g = L.EnsembleGrads()
        g.dlogits[0], g.dlogits[1] = alias, 0x200000
        assert call(grads=g) == 1, hex(alias)
    # entries [G, 8) are ignored, and with every entry null nothing is launched: the call returns
    none = L.EnsembleGrads()
    none.dlogits[2] = 0x20000
    assert call(grads=none) == 0
    with pytest.raises(ValueError, match=NAME):
        L.check(call(G=9), NAME)


# ------------------------------------------------------------------------ Python validation
def test_differentiable_must_be_a_bool_before_any_device_call():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError, match="differentiable"):
            S.ensemble_log_probs([x, x], differentiable=bad)
    with pytest.raises(TypeError):
        S.ensemble_log_probs([x, x], None, "prob", True)  # keyword-only
    for flag in (False, True):  # valid: the call goes on to the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.ensemble_log_probs([x, x], differentiable=flag)
    assert hasattr(S, "EnsembleLogProbsOp")


def test_mwer_takes_an_ensemble_spec_as_a_head():
    import scattennet_amd as S
    spec = S.EnsembleSpec(("left", "right", "body"), mode="logprob")
    m = S.MWER(0.5, 4, 3, reference=True, head=spec)
    assert m.head is spec and m.heads == (spec,)
    assert "EnsembleSpec(members=('left', 'right', 'body')" in repr(m) and "mode='logprob'" in repr(m)
    other = S.EnsembleSpec(("left", "right", "body"), mode="logprob")  # an equal spec, another object
    mixed = S.MWER(0.5, head=("fuse_coord_gloss_logits", spec, "left", other))
    assert mixed.heads == ("fuse_coord_gloss_logits", spec, "left", other) and isinstance(mixed.head, tuple)
    assert S.MWER(0.5, head=[spec]).heads == (spec,)
    eight = tuple(S.EnsembleSpec(("left",)) for _ in range(8))
    assert len(S.MWER(0.5, head=eight).heads) == 8
    with pytest.raises(ValueError, match="distinct"):
        S.MWER(0.5, head=(spec, spec))
    with pytest.raises(ValueError, match="distinct"):
        S.MWER(0.5, head=("left", spec, "left"))
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.MWER(0.5, head=eight + (spec,))
    for bad in (object(), ("left", "right"), 3, None, {"ensemble_gloss_logits": spec}):
        with pytest.raises(ValueError, match="head"):
            S.MWER(0.5, head=(spec, bad))
    with pytest.raises(ValueError, match="head"):
        S.MWER(0.5, head=object())
    # keys alone: as before
    assert S.MWER(0.5).heads == ("fuse_coord_gloss_logits",) and "EnsembleSpec" not in repr(S.MWER(0.5))
    assert S.MWER(0.5, head=("left", "right")).heads == ("left", "right")


def test_ensemble_spec_compute_passes_the_flag_on(monkeypatch):
    import scattennet_amd as S
    from scattennet_amd import ensemble as E
    seen = []

    def fake(xs, weights, mode, *, differentiable=False):
        seen.append((list(xs), weights, mode, differentiable))
        return "e"
    monkeypatch.setattr(E, "ensemble_log_probs", fake)
    spec = S.EnsembleSpec(("left", "body"), weights=[1, 3], mode="logprob")
    outputs = {"left": 1, "right": 2, "body": 3}
    assert spec.compute(outputs) == "e" and spec.compute(outputs, differentiable=True) == "e"
    assert seen[0] == ([1, 3], spec.weights, "logprob", False) and seen[1][3] is True
