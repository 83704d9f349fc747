"""GPU parity of the MWER loss (scattennet_amd/mwer.py: one op over sca_mwer_heads_fwd /
sca_mwer_heads_bwd) against the float64 restatement of tests/mwer_ref.py, under the project's
bound of 1e-3 (golden_util.rel_err); integers are compared as integers.  The kernels on the four
n-best cases in all four modes (plain, and with the reference slot and the prior, whose other
tests are tests/test_gpu_mwer_ext.py's; the helpers of both are tests/mwer_gpu.py) and on a
hand-built case, the single-tensor C entry points sca_mwer_fwd / sca_mwer_bwd against the one
path, the decode-and-loss entry point, capture, and the training steps on
tests/golden/model_small.  Every test prints the figures it asserts."""
import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import nbest_ref as NR
from tests.golden_util import close, rel_err
from tests.mwer_gpu import fx  # noqa: F401  (the fixture, by name)
from tests.mwer_gpu import (IDS, MODES, SHAPES, TOL, _assert_parity, _bits, _build, _case, _case_run, _dev, _grads, _nbest,
                            _run, _same, _trainer)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1: the kernels
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernels_against_the_restatement(shape, mode):
    B, T, C, W, N = shape
    with_ref, table = MODES[mode]
    (_, in_len, lists, _), want, _ = _case(shape, mode)
    if mode == "plain":
        for b in range(B):  # the conditions tests/test_mwer.py asserts on these inputs
            if in_len[b] >= 1:
                errs = want["errors"][b, :len(lists[b])]
                assert errs.min() != errs.max() and np.abs(want["dlogits"][b]).max() >= 1e-3
    loss, det, dx = _case_run(shape, mode)
    assert det["loglik"].shape == (B, N + with_ref) and ("ref_valid" in det) == with_ref and loss.dim() == 0
    _assert_parity(f"{IDS[SHAPES.index(shape)]} {mode}", loss, det, dx, want)
    assert np.abs(want["dlogits"]).max() >= 1e-3  # not a vacuous case
    for b in range(B):
        assert not dx[b, in_len[b]:].any(), b  # rows past in_len are written as zeros


# ------------------------------------------------------------------ 2: the hand-built case
def _hand_case():
    """B = 3, T = 10, C = 9, N = 4, H = 10.  Clip 0 (in_len 10, count 4): a genuine repeat (3, 3),
    the empty hypothesis among non-empty ones, an entry equal to the reference, and frame 4 with
    the logit of label 5 more than 100 below the row maximum (the clamp gate).  Clip 1 (in_len 3,
    count 3 < N, garbage in the unused entry, ref_len 0): (2, 2, 4) needs 4 frames and does not
    fit.  Clip 2 (in_len 6, count 3 < N): every entry is one substitution from the reference."""
    x = np.random.default_rng(5).normal(0.0, 1.0, (3, 10, 9)).astype(np.float32)
    x[0, 4, 5] = x[0, 4].max() - 130.0
    lists = [[[3, 3, 5], [], [3, 5], [7, 5, 1]], [[2], [2, 2, 4], [6, 1]], [[1, 2], [1, 3], [4, 8]]]
    refs = [[3, 5], [], [1, 8]]
    return x, [10, 3, 6], lists, refs


def test_hand_built_case():
    dev = _dev()
    x, in_len, lists, refs = _hand_case()
    want = M.mwer(x, in_len, lists, refs, 1.0, n_max=4)
    assert want["errors"][0].tolist() == [1, 2, 0, 2] and set(want["errors"][2, :3]) == {1}
    assert np.isneginf(want["loglik"][1, 1]) and np.isfinite(want["loglik"][1, [0, 2]]).all()
    raw = torch.log_softmax(torch.from_numpy(x[0, 4]).double(), -1)
    assert raw[5] < -100.0 and abs(want["dlogits"][0, 4, 5]) < 1e-40  # gated: only the softmax term, ~exp(-130)
    loss, det, dx = _run(x, in_len, lists, refs, 4, 10, dev, 1.0, fill=-7)
    _assert_parity("hand-built", loss, det, dx, want)
    assert float(det["posterior"][1, 1]) == 0.0 and float(det["posterior"][1, 3]) == 0.0
    assert not _bits(dx[2]).any(), "equal error counts: the gradient rows are exactly 0"
    assert not dx[1, 3:].any() and dx[1, :3].abs().max() > 0  # the unfit entry aside, clip 1 has a gradient
    assert float(dx[0, 4, 5].abs()) < 1e-30
    assert float(det["errors"][1, 3]) == 0 and np.isneginf(float(det["loglik"][1, 3]))


# ------------------------------------------------------------------ 3: the grid form
def _many_clips():
    """B = 70, T = 5, C = 4, N = 3, lengths ragged from 0, lists of 1 to 3 entries."""
    rng = np.random.default_rng(11)
    B, T, C, N = 70, 5, 4, 3
    x = rng.normal(0.0, 2.0, (B, T, C)).astype(np.float32)
    in_len = [int(v) for v in rng.integers(0, T + 1, B)]
    pool = [[1], [2, 3], [], [1, 1], [3, 2, 1], [2]]
    lists = [[pool[(b + k) % len(pool)] for k in range(1 + b % N)] for b in range(B)]
    refs = [pool[(b + 1) % len(pool)] for b in range(B)]
    return x, in_len, lists, refs


def test_many_clips_take_the_grid_form_of_the_per_clip_kernel():
    """B = 70 > 64: four clips per workgroup and the separate fixed-order sum over the clips."""
    dev = _dev()
    x, in_len, lists, refs = _many_clips()
    want = M.mwer(x, in_len, lists, refs, 1.0, n_max=3)
    assert np.abs(want["dlogits"]).max() >= 1e-3 and abs(want["loss"]) > 1e-3
    loss, det, dx = _run(x, in_len, lists, refs, 3, 5, dev, 1.0, fill=-3)
    _assert_parity("B70", loss, det, dx, want)


# ------------------------------------------------------------------ 4: the old entry points
def _case_of(shape, fill):
    logits, in_len, lists, refs = M.case_inputs(shape)
    return logits, in_len, lists, refs, shape[4], shape[1], M.POSTERIOR_SCALE, fill


# (logits, in_len, lists, refs, N, H, posterior_scale, fill): the smallest inputs that reach every
# branch of the launcher behind sca_mwer_fwd / sca_mwer_bwd
SINGLE_TENSOR_CASES = {
    "fill_behind_count_and_lengths": lambda: _case_of((4, 12, 6, 8, 3), -5),
    "ragged_lengths": lambda: _case_of((5, 16, 4, 8, 8), 0),
    "N32_all_lanes_of_the_clip_kernel": lambda: _case_of((3, 20, 33, 32, 32), 0),
    "hand_built_clamp_gate_unfit_entry_empty_reference": lambda: _hand_case() + (4, 10, 1.0, -7),
    "B70_grid_form_and_loss_sum_kernel": lambda: _many_clips() + (3, 5, 1.0, -3),
}


@pytest.mark.parametrize("case", list(SINGLE_TENSOR_CASES))
def test_single_tensor_entry_points_are_the_one_path(case):
    """sca_mwer_workspace_floats / sca_mwer_fwd / sca_mwer_bwd, which no Python of the package
    calls, through the library on device tensors: the loss, every detail and dlogits are bitwise
    what `mwer_loss` (sca_mwer_heads_fwd / sca_mwer_heads_bwd at G = 1) gives."""
    import scattennet_amd as S
    from scattennet_amd import _lib as L
    dev = _dev()
    logits, in_len, lists, refs, N, H, ps, fill = SINGLE_TENSOR_CASES[case]()
    B, T, C = logits.shape
    nb = _nbest(lists, N, H, dev, fill)
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    ref, ref_len = (torch.from_numpy(a).to(dev) for a in M.pack_refs(refs))
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    loss, det = S.mwer_loss(x, il, ref, ref_len, nbest=nb, posterior_scale=ps, return_details=True)
    loss.backward()
    assert loss.dim() == 0 and set(det) == {"loglik", "posterior", "errors", "risk"}
    lib, xd = L.lib(), x.detach()
    ws = xd.new_empty(max(lib.sca_mwer_workspace_floats(B, N, T, H), 1))
    old_loss, dloss, dx = xd.new_empty(()), xd.new_ones(()), torch.empty_like(xd)
    old = {"loglik": xd.new_empty(B, N), "posterior": xd.new_empty(B, N),
           "errors": torch.empty(B, N, dtype=torch.int32, device=dev), "risk": xd.new_empty(B)}
    L.check(lib.sca_mwer_fwd(L.ptr(xd), L.ptr(il), L.ptr(nb.tokens), L.ptr(nb.lengths), L.ptr(nb.count), L.ptr(ref),
                             L.ptr(ref_len), B, N, T, C, H, ref.shape[1], ps, L.ptr(old["loglik"]),
                             L.ptr(old["posterior"]), L.ptr(old["errors"]), L.ptr(old["risk"]), L.ptr(old_loss),
                             L.ptr(ws), L.stream_handle()), "sca_mwer_fwd")
    L.check(lib.sca_mwer_bwd(L.ptr(xd), L.ptr(il), L.ptr(nb.tokens), L.ptr(nb.lengths), L.ptr(nb.count), B, N, T, C, H,
                             L.ptr(dloss), L.ptr(ws), L.ptr(dx), L.stream_handle()), "sca_mwer_bwd")
    torch.cuda.synchronize()
    _same((old_loss, old, dx), (loss.detach(), det, x.grad), case)
    print(case, "loss", float(old_loss), "max |dlogits|", float(dx.abs().max()))
    assert dx.abs().max() > 0


# ------------------------------------------------------------------ 5: end to end
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_decode_and_loss_against_the_restatement(shape):
    import scattennet_amd as S
    dev = _dev()
    B, T, C, W, N = shape
    logits, in_len, lists, refs = M.case_inputs(shape)
    want = M.case_ref(shape)
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    ref, ref_len = M.pack_refs(refs)
    loss, det = S.mwer_loss(x, torch.tensor(in_len), torch.from_numpy(ref), torch.from_numpy(ref_len), beam_size=W,
                            nbest_size=N, posterior_scale=M.POSTERIOR_SCALE, return_details=True)
    loss.backward()
    torch.cuda.synchronize()
    _assert_parity("end to end " + IDS[SHAPES.index(shape)], loss.detach().cpu(), {k: v.cpu() for k, v in det.items()},
                   x.grad.cpu(), want)


# ------------------------------------------------------------------ 6: capture
def test_captured_forward_and_backward_replay_bitwise():
    import scattennet_amd as S
    dev = _dev()
    shape = (5, 16, 4, 8, 8)
    B, T, C, W, N = shape
    logits, in_len, lists, refs = M.case_inputs(shape)
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    ref, ref_len = (torch.from_numpy(a).to(dev) for a in M.pack_refs(refs))

    def chain():
        x.grad = None
        loss, det = S.mwer_loss(x, il, ref, ref_len, beam_size=W, nbest_size=N, posterior_scale=M.POSTERIOR_SCALE,
                                return_details=True)
        loss.backward()
        return [loss.detach(), det["loglik"], det["posterior"], det["errors"], det["risk"], x.grad]

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
                x.copy_(torch.from_numpy(np.random.default_rng(seed).normal(0.0, 4.0, (B, T, C)).astype(np.float32)))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        for i, (a, b) in enumerate(zip(got, chain())):
            assert torch.equal(_bits(a), _bits(b)), (seed, i)
        assert got[5].abs().max() > 0


# ------------------------------------------------------------------ 7: the steps
HEAD = "fuse_coord_gloss_logits"
BEAM, NBEST, WEIGHT = NR.MODEL_BEAM, 3, 0.5


def _spec():
    import scattennet_amd as S
    return S.MWER(weight=WEIGHT, beam_size=BEAM, nbest=NBEST)


def _restated(out, src):
    """The restatement on the step's own logits, lists from the restatement's search."""
    logits = out[HEAD].detach().double().cpu().numpy()
    lens = out["input_lengths"].cpu().numpy()
    lists = []
    for b in range(len(logits)):
        entries, gaps = NR.nbest(logits[b], lens[b], BEAM, NBEST, collapse_repeats=False)
        assert min(gaps["frame"], gaps["final"]) >= 1e-4, gaps  # no tie in the search (tests/test_nbest.py)
        lists.append([h for h, _ in entries])
    lab, ll = src["gloss_labels"].cpu().numpy(), src["gloss_lengths"].cpu().numpy()
    refs = [lab[b, :ll[b]].tolist() for b in range(len(logits))]
    return M.mwer(logits, lens, lists, refs, 1.0, n_max=NBEST)


@pytest.fixture(scope="module")
def eager(fx):
    """One eager step with MWER and one without on twin models, computed once."""
    import scattennet_amd as S
    dev = _dev()
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    model, opt = _trainer(fx, dev)
    out = S.train_step(model, opt, src, mwer=_spec())
    rep = S.read_report(out)
    with_mwer = ({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in out.items()}, _grads(model), rep)
    plain_model, plain_opt = _trainer(fx, dev)
    plain_out = S.train_step(plain_model, plain_opt, src)
    plain = ({k: v.detach().cpu() if torch.is_tensor(v) else v for k, v in plain_out.items()}, _grads(plain_model),
             S.read_report(plain_out))
    return {"src": src, "mwer": with_mwer, "plain": plain, "want": _restated(with_mwer[0], src)}


def test_step_loss_and_gradients_against_the_restatement(fx, eager):
    dev = _dev()
    out, grads, rep = eager["mwer"]
    plain_out, plain_grads, plain_rep = eager["plain"]
    want = eager["want"]
    errs = want["errors"]
    print("mwer_loss", float(out["mwer_loss"]), "restated", want["loss"], "errors", errs.tolist(), "max |dlogits_ref|",
          np.abs(want["dlogits"]).max())
    assert any(e.min() != e.max() for e in errs) and np.abs(want["dlogits"]).max() >= 1e-3  # not a vacuous case
    assert rel_err(out["mwer_loss"], torch.tensor(want["loss"])) < TOL
    assert rel_err(out["mwer_risk"], torch.from_numpy(want["risk"])) < TOL
    # the parameter gradients minus those of the mwer=None step = WEIGHT * dlogits_ref through the head
    model = _build(fx, dev)
    logits = model(eager["src"])[HEAD]
    logits.backward(torch.from_numpy(WEIGHT * want["dlogits"]).float().to(dev))
    torch.cuda.synchronize()
    ref_grads = _grads(model)
    gscale = max(float(g.abs().max()) for g in ref_grads.values() if g is not None)
    worst = 0.0
    for k, g in ref_grads.items():
        if g is None:
            continue
        diff = grads[k] - plain_grads[k]
        if float(g.abs().max()) >= 1e-4 * gscale:
            worst = max(worst, rel_err(diff, g))
        assert close(diff, g, TOL, gscale), (k, rel_err(diff, g))
    print("parameter gradients: worst rel_err", worst, "gradient scale", gscale)
    # the report: the two new numbers, from the one copy; the parent's keys without MWER
    assert abs(rep["mwer_loss"] - float(out["mwer_loss"])) == 0.0 and rep["skipped"] is False
    assert abs(rep["mwer_risk"] - float(out["mwer_risk"].mean())) < 1e-6
    assert rel_err(torch.tensor(rep["total_loss"]), torch.tensor(plain_rep["total_loss"])) < 1e-6
    assert set(out) - set(plain_out) == {"mwer_loss", "mwer_risk", "mwer_report"}
    assert "mwer_loss" not in plain_rep and set(plain_out) == set(model(eager["src"]))  # the forward's own keys


def test_guard_is_nan_for_a_non_finite_loss():
    import scattennet_amd as S
    dev = _dev()
    guard = torch.tensor(1.25, device=dev)
    assert float(S.mwer_guard(guard, torch.tensor(0.5, device=dev))) == 1.25
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert torch.isnan(S.mwer_guard(guard, torch.tensor(bad, device=dev)))
    assert torch.isnan(S.mwer_guard(torch.tensor(float("nan"), device=dev), torch.tensor(0.5, device=dev)))


def test_bucketed_step_equals_the_eager_unpadded_step(fx, eager):
    import scattennet_amd as S
    dev = _dev()
    out, grads, rep = eager["mwer"]
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3, mwer=_spec())
    gscale = max(float(g.abs().max()) for g in grads.values() if g is not None)
    for use in ("eager first use", "capture and replay", "replay"):
        got = bts.step(eager["src"])
        got_rep = S.read_report(got)
        torch.cuda.synchronize()
        assert bts.graphs_captured == (0 if use == "eager first use" else 1)
        figs = {k: rel_err(torch.tensor(got_rep[k]), torch.tensor(rep[k])) for k in ("total_loss", "mwer_loss", "mwer_risk")}
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
        assert got[HEAD].shape[1] == 13
