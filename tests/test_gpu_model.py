"""MSCA_Net on the MI355X: the finite scan against torch.isnan / torch.isinf, forward and
backward parity with the reference's whole-model fixture (model_small), the reference's
ValueErrors from the device-side guard, decoding of the outputs, and the training step
(eager and as one captured hipGraph) against the reference's recorded six-step trajectory."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests.golden_util import close, load, load_arrays, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's parity bound (relative fp32)
LOGITS = ["alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits"]
LOSSES = ["total_loss", "alignment_loss", "fuse_coord_loss", "left_distill_loss", "right_distill_loss",
          "body_distill_loss"]
NAN_BITS = [0x7fc00001, 0xffc12345, 0x7f800001, 0xff8fffff]  # either sign, quiet / signalling, payloads
INF_BITS = [0x7f800000, 0xff800000]
FINE_BITS = [0x00000001, 0x807fffff, 0x80000000, 0x7f7fffff, 0xff7fffff, 0x00800000]  # denormals, -0, +-FLT_MAX


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(v):
    return np.array([v], dtype=np.uint32).view(np.float32)[0]


def _expected(a):
    t = torch.from_numpy(a)
    return int(bool(torch.isnan(t).any())) | (int(bool(torch.isinf(t).any())) << 1)


def _place(a, dev, offset):
    """`a` on the device, starting `offset` floats past a 16-byte boundary (a contiguous view)."""
    base = torch.zeros(a.size + offset + 4, dtype=torch.float32, device=dev)
    view = base[offset:offset + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.is_contiguous() and (a.size == 0 or view.data_ptr() % 16 == 4 * (offset % 4))
    return view


# ------------------------------------------------------------------ 1: the scan
def _scan_cases():
    from scattennet_amd import _lib
    C = _lib.GUARD_CHUNK
    rng = np.random.default_rng(5)
    cases = []
    for n in [0, 1, 3, 5, 4097, C - 1, C, C + 1, 100003]:
        clean = rng.standard_normal(n).astype(np.float32)
        for i, b in enumerate(FINE_BITS):
            if n:
                clean[(i * 977) % n] = _bits(b)
        cases.append(clean)
        # first / last element, both sides of every chunk boundary in reach, and the elements a
        # view offset by one to three floats reads with 4-byte loads (head and tail)
        spots = sorted({p for p in [0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1, C - 1, C, 2 * C - 1, 2 * C, n // 2]
                        if 0 <= p < n})
        for j, p in enumerate(spots):
            a = clean.copy()
            a[p] = _bits((NAN_BITS + INF_BITS)[j % 6])
            cases.append(a)
        if n >= 2:
            a = clean.copy()
            a[0], a[n - 1] = _bits(NAN_BITS[1]), _bits(INF_BITS[1])  # both kinds in one tensor
            cases.append(a)
    return cases


def test_finite_flags_match_torch_at_every_alignment():
    import scattennet_amd as S
    dev = _dev()
    cases = _scan_cases()
    want = [_expected(a) for a in cases]
    assert {0, 1, 2, 3} <= set(want)
    got = []
    for offset in range(4):  # the same data at four alignments: the same words
        flags = S.finite_flags([_place(a, dev, offset) for a in cases])  # > 16 tensors: several launches
        assert flags.dtype == torch.int32 and flags.is_cuda and flags.shape == (len(cases),)
        got.append(flags.cpu().tolist())
    for offset in range(4):
        bad = [(i, cases[i].size, g, w) for i, (g, w) in enumerate(zip(got[offset], want)) if g != w]
        assert not bad, (offset, bad[:8])


def test_finite_flags_seventeen_tensors_and_shapes():
    import scattennet_amd as S
    dev = _dev()
    ts = [torch.full((3, 5), float(i), device=dev) for i in range(17)]
    ts[0][2, 4] = float("nan")
    ts[15][0, 0] = float("inf")
    ts[16][1, 1] = float("-inf")
    ts[16][1, 2] = float("nan")
    ts.append(torch.zeros((), device=dev))  # 0-d, as the loss terms are
    want = [1] + [0] * 14 + [2, 3, 0]
    assert S.finite_flags(ts).cpu().tolist() == want
    for t, w in zip(ts, want):
        assert w == int(bool(torch.isnan(t).any())) | (int(bool(torch.isinf(t).any())) << 1)


def test_finite_flags_bad_arguments():
    import scattennet_amd as S
    from scattennet_amd import _lib as L
    dev = _dev()
    x = torch.zeros(8, 8, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.finite_flags([x.half()])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.finite_flags([x, x.cpu()])
    with pytest.raises(ValueError, match="contiguous"):
        S.finite_flags([x[:, ::2]])
    flags = torch.zeros(32, dtype=torch.int32, device=dev)
    st = L.stream_handle()

    def scan(ptrs, numels):
        n = len(ptrs)
        return L.lib().sca_finite_scan(n, (ctypes.c_void_p * n)(*ptrs), (ctypes.c_long * n)(*numels), L.ptr(flags), st)

    assert scan([x.data_ptr()] * 17, [4] * 17) == 1       # more than 16 tensors
    assert scan([x.data_ptr(), None], [4, 4]) == 1          # null pointer with numel > 0
    assert scan([x.data_ptr()], [-1]) == 1                  # negative size
    assert scan([x.data_ptr(), None], [4, 0]) == 0          # an empty tensor needs no pointer
    with pytest.raises(ValueError, match="sca_finite_scan"):
        L.check(scan([x.data_ptr()], [-1]), "sca_finite_scan")
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0] * 32


# ------------------------------------------------------------------ 2: the model against the fixture
def _build(fx, dev, **over):
    import scattennet_amd as S
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    cfg.update(over)
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


@pytest.fixture(scope="module")
def ran(fx):
    """One forward + backward of the fixture's batch (host tensors in, as the reference's
    data loader hands them over; device="cuda" moves them)."""
    dev = _dev()
    model = _build(fx, dev)
    out = model(dict(fx["in"]))
    out["total_loss"].backward()
    torch.cuda.synchronize()
    return model, out


def test_forward_parity(fx, ran):
    _, out = ran
    z = load_arrays("model_small")
    assert set(out) == {k[4:] for k in z if k.startswith("out.")} | {"finite_report"}
    for k in LOGITS + LOSSES:
        ref = torch.from_numpy(z["out." + k])
        err = rel_err(out[k], ref)
        print(k, "rel_err", err)
        assert out[k].shape == ref.shape and close(out[k].detach().cpu(), ref, TOL), (k, err)
    assert out["input_lengths"].is_cuda and torch.equal(out["input_lengths"].cpu(), fx["in"]["valid_len_in"])
    assert out["finite_report"].dtype == torch.int32 and "loss" not in "finite_report"


def test_report_holds_the_losses_and_clean_flags(fx, ran):
    import scattennet_amd as S
    model, out = ran
    rep = S.read_report(out)
    assert rep["flags"] == [0] * 15 and rep["skipped"] is False
    for k in LOSSES:
        assert rep[k] == float(out[k].detach())  # the same fp32 values, bitwise
    assert rep["guard"] == rep["total_loss"]
    want = out["fuse_coord_loss"].detach().clone()
    for s in ("left", "right", "body"):  # the reference's order of additions (model/__init__.py:207,237)
        want = want + out[f"{s}_distill_loss"].detach()
    assert float(want) == rep["total_loss"]


def test_backward_parity(fx, ran):
    model, _ = ran
    gscale = max(float(g.abs().max()) for g in fx["grad_param"].values())
    named = dict(model.named_parameters())
    assert set(named) == set(fx["grad_param"]) | set(fx["meta"]["no_grad"])
    worst = ("", 0.0)
    for k, g in fx["grad_param"].items():
        got = named[k].grad
        assert got is not None, k
        err = rel_err(got.cpu(), g)
        if float(g.abs().max()) >= 1e-4 * gscale and err > worst[1]:
            worst = (k, err)
        assert close(got.cpu(), g, TOL, gscale), (k, err)
    print("worst gradient rel_err", worst)
    for k in fx["meta"]["no_grad"]:  # the alignment head: not in total_loss
        assert named[k].grad is None or float(named[k].grad.abs().max()) == 0.0, k


def test_without_self_distillation(fx):
    dev = _dev()
    model = _build(fx, dev, self_distillation=False)
    out = model(dict(fx["in"]))
    assert not [k for k in out if k.endswith("_distill_loss")]
    assert torch.equal(out["total_loss"].detach().view(torch.int32), out["fuse_coord_loss"].detach().view(torch.int32))
    assert out["finite_report"].numel() == 12 + 4
    z = load_arrays("model_small")
    assert close(out["fuse_coord_loss"].detach().cpu(), torch.from_numpy(z["out.fuse_coord_loss"]), TOL)
    out["total_loss"].backward()
    assert model.recognition_head.left_gloss_classifier.weight.grad is None
    assert model.recognition_head.fuse_coord_classifier.weight.grad is not None


def test_decode_outputs(fx, ran):
    import scattennet_amd as S
    _, out = ran
    dec = S.decode_outputs(out, beam_size=1)
    assert set(dec) == {"alignment_", "fuse_coord_"}  # one hypothesis list per *gloss_logits head
    for name, hyps in dec.items():
        assert len(hyps) == fx["meta"]["B"] and all(isinstance(h, list) for h in hyps)
        assert all(0 < c < fx["meta"]["vocab"] for h in hyps for c in h)
        assert hyps == S.ctc_decode(out[name + "gloss_logits"], 1, out["input_lengths"]), name


# ------------------------------------------------------------------ 3: non-finite handling
def _nan_keypoints(fx):
    src = dict(fx["in"])
    kp = src["keypoints"].clone()
    kp[1, 3, 6, 0] = float("nan")  # a valid frame of clip 1, a left-hand joint
    src["keypoints"] = kp
    return src


def test_nan_keypoint_raises_like_the_reference(fx, monkeypatch):
    import scattennet_amd.model as M
    dev = _dev()
    model = _build(fx, dev)
    src = _nan_keypoints(fx)
    assert model.check == "sync"
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        model(src)
    model.check = "defer"
    out = model(src)  # returns: nothing was read
    rep = M.read_report(out)
    assert rep["flags"][0] == 1 and rep["guard"] != rep["guard"]
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        model.raise_if_nonfinite(out)
    model.check = "off"
    monkeypatch.setattr(M, "finite_flags", lambda ts: pytest.fail("check='off' launched a scan"))
    out = model(src)
    assert model.raise_if_nonfinite(out)["flags"] == [0] * 15


def test_nan_classifier_bias_names_its_head(fx):
    dev = _dev()
    model = _build(fx, dev)
    with torch.no_grad():
        model.recognition_head.left_gloss_classifier.bias[2] = float("nan")
    with pytest.raises(ValueError, match="^NaN in left$"):
        model(dict(fx["in"]))
    with torch.no_grad():
        model.recognition_head.left_gloss_classifier.bias[2] = 0.0
        model.recognition_head.right_gloss_classifier.bias[0] = float("inf")
    # clamp(+inf) is 50 (model/__init__.py:57): nothing to flag, as in the reference
    assert model.raise_if_nonfinite(model(dict(fx["in"])))["flags"] == [0] * 15


def test_deferred_forward_under_stream_capture(fx):
    """A host read would abort the capture: "sync" must behave as "defer" while capturing."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = {k: v.to(dev) for k, v in fx["in"].items()}
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        model(src)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = model(src)  # check == "sync"
    graph.replay()
    rep = S.read_report(out)
    z = load_arrays("model_small")
    assert rep["flags"] == [0] * 15 and abs(rep["total_loss"] - float(z["out.total_loss"])) < TOL * rep["total_loss"]
    src["keypoints"][1, 3, 6, 0] = float("nan")  # the graph reads the same storage
    graph.replay()
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        S.read_report(out)


# ------------------------------------------------------------------ 4: the training step
ADAM = dict(lr=2e-3, betas=(0.9, 0.998), weight_decay=2e-5)


def _trainer(fx, dev):
    import scattennet_amd as S
    model = _build(fx, dev)
    opt = S.FusedAdam(model.parameters(), max_grad_norm=model.gradient_clip_val, **ADAM)
    return model, opt, {k: v.to(dev) for k, v in fx["in"].items()}


def _check_trajectory(label, losses, norms):
    z = load_arrays("model_small")
    ref_l, ref_n = z["train.total_loss"], z["train.grad_norm"]
    el = np.abs(np.array(losses) - ref_l) / np.abs(ref_l)
    en = np.abs(np.array(norms) - ref_n) / np.abs(ref_n)
    print(label, "loss", losses, "rel", el.tolist(), "norm", norms, "rel", en.tolist())
    assert len(losses) == 6 and el.max() < TOL and en.max() < TOL, (label, el.tolist(), en.tolist())


def test_train_step_eager_follows_the_reference(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt, src = _trainer(fx, dev)
    losses, norms = [], []
    for _ in range(6):
        out = S.train_step(model, opt, src)
        rep = S.read_report(out)
        assert rep["skipped"] is False and model.check == "sync"
        losses.append(rep["total_loss"])
        norms.append(float(opt.grad_norm))
    assert int(opt.step_count) == 6 and int(opt.skipped) == 0
    _check_trajectory("eager", losses, norms)


def test_train_step_captured_follows_the_reference(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt, src = _trainer(fx, dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        out = S.train_step(model, opt, src)  # eager warm-up: step 1
    torch.cuda.current_stream().wait_stream(s)
    rep = S.read_report(out)
    losses, norms = [rep["total_loss"]], [float(opt.grad_norm)]
    del out  # a captured backward must not find the warm-up step's autograd graph alive
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.train_step(model, opt, src)
    for _ in range(5):
        opt.sync_hyperparameters()
        graph.replay()
        rep = S.read_report(out)
        losses.append(rep["total_loss"])
        norms.append(float(opt.grad_norm))
    assert int(opt.step_count) == 6
    _check_trajectory("captured", losses, norms)


def _state_bits(model, opt):
    ts = [p.detach() for p in model.parameters()]
    for p in model.parameters():
        st = opt.state.get(p, {})
        ts += [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
    return [t.clone().view(torch.int32) for t in ts]


@pytest.mark.parametrize("where", ["keypoints", "alignment_bias"])
def test_train_step_skips_on_nonfinite(fx, where):
    """The update is skipped on the device — also when the flagged tensor does not feed
    total_loss (the alignment head): `guard` covers every checked tensor."""
    import scattennet_amd as S
    dev = _dev()
    model, opt, src = _trainer(fx, dev)
    S.read_report(S.train_step(model, opt, src))  # a good step: the moments exist
    if where == "keypoints":
        src = {k: v.to(dev) for k, v in _nan_keypoints(fx).items()}
        message = "^NaN or inf in input keypoints$"
    else:
        with torch.no_grad():
            model.recognition_head.fuse_alignment_head.gloss_layer.bias[1] = float("nan")
        message = "^NaN in alignment_gloss_logits$"
    before = _state_bits(model, opt)
    assert len(before) > 100
    out = S.train_step(model, opt, src)
    assert int(opt.skipped) == 1 and int(opt.step_count) == 1
    after = _state_bits(model, opt)
    assert len(after) == len(before) and all(torch.equal(a, b) for a, b in zip(after, before))
    if where == "alignment_bias":  # total_loss itself is fine: only the guard stops the update
        assert bool(torch.isfinite(out["total_loss"]))
    with pytest.raises(ValueError, match=message):
        S.read_report(out)
