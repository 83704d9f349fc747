"""What tests/test_gpu_mwer.py and tests/test_gpu_mwer_ext.py share: the cases' constants, the
MWER loss on host inputs, the parity and bitwise assertions, one cached GPU run per (case, mode),
and the fixture model of the step tests."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import nbest_ref as NR
from tests.golden_util import load, rel_err

TOL = 1e-3  # the project's relative bound
SHAPES = list(NR.CASES)
IDS = ["B%d_T%d_C%d_W%d_N%d" % s for s in SHAPES]
# (with_ref, table); "plain" runs on the references of M.case_inputs, the others on M.case_inputs_ext's
MODES = {"plain": (False, False), "reference+table": (True, True), "reference": (True, False), "table": (False, True)}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nbest(lists, N, H, dev, fill=0):
    """An NBest from host lists: one head's (lists[b]) or, for a tuple of G of them, the heads' form."""
    import scattennet_amd as S
    if isinstance(lists, tuple):
        tokens, out_len, count = (np.stack(a) for a in zip(*(M.pack_lists(l, N, H, fill) for l in lists)))
    else:
        tokens, out_len, count = M.pack_lists(lists, N, H, fill)
    return S.NBest(torch.from_numpy(tokens).to(dev), torch.from_numpy(out_len).to(dev),
                   torch.zeros(out_len.shape, device=dev), torch.from_numpy(count).to(dev))


def _lm(table, dev):
    import scattennet_amd as S
    return None if table is None else S.BigramLM(torch.from_numpy(np.asarray(table)), dev)


def _run(logits, in_len, lists, refs, N, H, dev, ps, fill=0, lm=None, **kw):
    """The op on host inputs: (loss, details, dlogits) as host tensors.  `logits` / `lists`: one
    head's, or tuples of G of them (dlogits is then a list)."""
    import scattennet_amd as S
    grouped = isinstance(logits, tuple)
    xs = [torch.from_numpy(np.asarray(x, np.float32)).to(dev).requires_grad_(True) for x in (logits if grouped else (logits,))]
    ref, ref_len = M.pack_refs(refs)
    loss, det = S.mwer_loss(xs if grouped else xs[0], torch.tensor(in_len), torch.from_numpy(ref),
                            torch.from_numpy(ref_len), nbest=_nbest(lists, N, H, dev, fill), posterior_scale=ps,
                            return_details=True, lm=_lm(lm, dev), **kw)
    loss.sum().backward()
    torch.cuda.synchronize()
    grads = [x.grad.cpu() for x in xs]
    return loss.detach().cpu(), {k: v.cpu() for k, v in det.items()}, grads if grouped else grads[0]


def _assert_parity(where, loss, det, dx, want):
    """Every output against the restatement; returns the measured figures."""
    ll, wl = det["loglik"].double().numpy(), want["loglik"]
    assert np.array_equal(np.isneginf(ll), np.isneginf(wl)), (where, ll, wl)
    fin = np.isfinite(wl)
    figs = {"loglik": rel_err(torch.from_numpy(ll[fin]), torch.from_numpy(wl[fin])),
            "posterior": rel_err(det["posterior"], torch.from_numpy(want["posterior"])),
            "risk": rel_err(det["risk"], torch.from_numpy(want["risk"])),
            "loss": rel_err(loss, torch.tensor(want["loss"])),
            "dlogits": rel_err(dx, torch.from_numpy(want["dlogits"]))}
    print(where, {k: f"{v:.3g}" for k, v in figs.items()}, "loss", want["loss"])
    assert np.array_equal(det["errors"].numpy().astype(np.int64), want["errors"]), where
    if "ref_valid" in det:
        assert np.array_equal(det["ref_valid"].numpy().astype(np.int64), want["ref_valid"]), where
    for k, v in figs.items():
        assert v < TOL, (where, k, v)
    return figs


def _case(shape, mode):
    """(inputs, restatement, the call's keywords) of a case in a mode."""
    with_ref, table = MODES[mode]
    if mode == "plain":
        return M.case_inputs(shape), M.case_ref(shape), {}
    kw = dict(reference=with_ref, **M.prior_kwargs(shape, table))
    return M.case_inputs_ext(shape), M.case_ref_ext(shape, with_ref, table), kw


@functools.lru_cache(maxsize=None)
def _case_run(shape, mode):
    """One GPU run of a case in a mode, shared by the tests that read it."""
    (logits, in_len, lists, refs), _, kw = _case(shape, mode)
    return _run(logits, in_len, lists, refs, shape[4], shape[1], _dev(), M.POSTERIOR_SCALE, **kw)


def _same(a, b, where):
    (la, da, ga), (lb, db, gb) = a, b
    assert torch.equal(_bits(la), _bits(lb)), where
    assert set(da) == set(db)
    for k in da:
        assert da[k].dtype == db[k].dtype and torch.equal(_bits(da[k]), _bits(db[k])), (where, k)
    assert torch.equal(_bits(ga), _bits(gb)), where


# ------------------------------------------------------------------ the steps
ADAM = dict(lr=0.0, betas=(0.9, 0.998), weight_decay=0.0)  # lr 0: every step sees the same parameters


@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


def _build(fx, dev):
    """The dropout-free configuration of the existing step tests: the fixture model in eval mode."""
    import scattennet_amd as S
    m = S.MSCA_Net(copy.deepcopy(fx["meta"]["cfg"]), list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


def _trainer(fx, dev):
    import scattennet_amd as S
    model = _build(fx, dev)
    return model, S.FusedAdam(model.parameters(), **ADAM)


def _grads(model):
    return {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in model.named_parameters()}
