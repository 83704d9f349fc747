"""Length buckets on the MI355X: the three valid-frame kernels against torch on the valid slice
(F.softmax, nn.KLDivLoss, nn.LSTM — the reference's own arithmetic), and MSCA_Net /
BucketedTrainStep on padded batches against the reference's whole-model fixture and against
the unpadded eager path.

"Bitwise 0" below means the int32 view is 0 where a kernel stores the zero itself (softmax
forward, SeqKD backward, the LSTM's states).  Where a zero comes out of a product — the
softmax backward's y * (dy - sum) with y = 0, a GEMM over zero gate gradients — its sign bit
follows the other factor, so those are asserted to be exact zeros (== 0, which -0.0 is)."""
import copy

import numpy as np
import pytest
import torch

from tests.golden_util import close, load, load_arrays, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's parity bound (relative fp32), as tests/test_gpu_model.py applies it
PARITY_TOL = 1e-3  # tests/test_gpu_wide_rows.py, the unrestricted row softmax
LOSS_TOL = dict(rtol=1e-5, atol=1e-4)  # tests/test_heads.py, SeqKD
GRAD_TOL = dict(rtol=1e-4, atol=2e-5)
ALIGN_TOL = dict(rtol=1e-4, atol=2e-5)  # tests/test_heads.py, the alignment head (out: atol 1e-5)
LOGITS = ["alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits"]
LOSSES = ["total_loss", "alignment_loss", "fuse_coord_loss", "left_distill_loss", "right_distill_loss",
          "body_distill_loss"]
ADAM = dict(lr=2e-3, betas=(0.9, 0.998), weight_decay=2e-5)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits_zero(t):
    return t.numel() == 0 or not bool(t.contiguous().view(torch.int32).any())


def _exact_zero(t):
    return not bool((t != 0).any())


def _valid(dev, nv, shift):
    """The device scalar for a valid length nv at the op; shift 2 stores 4 nv + 3 (the floor)."""
    return torch.tensor([nv if shift == 0 else (nv << shift) + (1 << shift) - 1], dtype=torch.int32, device=dev)


# ------------------------------------------------------------------ 1: softmax
@pytest.mark.parametrize("shift", [0, 2])
@pytest.mark.parametrize("N", [16, 100, 256, 1040])  # generic register form, NV = 1 form, wide form
def test_softmax_rows_valid(N, shift):
    import scattennet_amd  # noqa: F401
    dev = _dev()
    g = torch.Generator().manual_seed(N)
    x = (3 * torch.randn(2, 5, N, generator=g)).to(dev)
    dy = torch.randn(2, 5, N, generator=g).to(dev)
    full = torch.ops.scatten.softmax_rows(x)
    results = {}
    for nv in (1, N // 2 + 1, N - 1, N):
        vf = _valid(dev, nv, shift)
        xg = x.clone().requires_grad_(True)
        y = torch.ops.scatten.softmax_rows_valid(xg, vf, shift)
        y.backward(dy)
        xr = x[..., :nv].clone().requires_grad_(True)
        ref = torch.softmax(xr, dim=-1)
        ref.backward(dy[..., :nv])
        ey, ex = rel_err(y[..., :nv], ref), rel_err(xg.grad[..., :nv], xr.grad)
        print(f"N={N} shift={shift} nv={nv}: y rel_err {ey:.3g}, dx rel_err {ex:.3g}")
        assert ey < PARITY_TOL and ex < PARITY_TOL
        assert _bits_zero(y.detach()[..., nv:])
        assert _exact_zero(xg.grad[..., nv:]) and bool(torch.isfinite(xg.grad).all())
        if nv == N:
            assert torch.equal(y.detach().view(torch.int32), full.view(torch.int32))
        results[nv] = y.detach().clone()
    # the scalar is read on the device: same tensors, same host arguments, another value in memory
    vf = _valid(dev, N, shift)
    a = torch.ops.scatten.softmax_rows_valid(x, vf, shift).clone()
    vf.copy_(_valid(dev, N // 2 + 1, shift))
    b = torch.ops.scatten.softmax_rows_valid(x, vf, shift)
    assert torch.equal(a, results[N]) and torch.equal(b, results[N // 2 + 1]) and not torch.equal(a, b)


def test_softmax_rows_valid_clamps_a_bad_scalar():
    import scattennet_amd  # noqa: F401
    dev = _dev()
    x = torch.randn(3, 40, device=dev)
    for bad, like in ((0, 1), (-7, 1), (1 << 20, 40)):
        y = torch.ops.scatten.softmax_rows_valid(x, torch.tensor([bad], dtype=torch.int32, device=dev), 0)
        want = torch.ops.scatten.softmax_rows_valid(x, torch.tensor([like], dtype=torch.int32, device=dev), 0)
        assert torch.equal(y, want)
    with pytest.raises(ValueError, match="int32 device tensor"):
        torch.ops.scatten.softmax_rows_valid(x, torch.tensor([3], device=dev), 0)  # int64


# ------------------------------------------------------------------ 2: SeqKD
def _kd_reference(s, q, nv, weight, start=1):
    """loss.py:5-21 + model/__init__.py:203-214 on the rows t < nv, in torch on the CPU."""
    s = s.detach().cpu()[:, :nv].clone().requires_grad_(True)
    q = q.detach().cpu()[:, :nv].clone().requires_grad_(True)
    C = s.shape[-1] - start
    pred = torch.log_softmax(s[:, :, start:], dim=-1).view(-1, C)
    ref = torch.softmax(q[:, :, start:], dim=-1).view(-1, C)
    loss = torch.clamp(weight * torch.nn.KLDivLoss(reduction="batchmean")(pred, ref), -100, 100)
    loss.backward()
    return loss.detach(), s.grad, q.grad


@pytest.mark.parametrize("nv", [1, 5, 8])
def test_seqkd_valid(nv):
    from scattennet_amd import heads
    dev = _dev()
    B, T, C, w = 3, 8, 12, 0.5
    g = torch.Generator().manual_seed(2)
    s0, q0 = 2 * torch.randn(B, T, C, generator=g), 2 * torch.randn(B, T, C, generator=g)
    for shift in (0, 2):
        vf = _valid(dev, nv, shift)
        s = s0.to(dev).requires_grad_(True)
        q = q0.to(dev).requires_grad_(True)
        loss = heads.distillation_loss(s, q, w, valid=(vf, shift))  # the teacher is detached, as in the model
        loss.backward()
        ref_loss, ref_ds, ref_dq = _kd_reference(s0, q0, nv, w)
        print(f"nv={nv} shift={shift}: loss {loss.item():.7g} ref {ref_loss.item():.7g}")
        np.testing.assert_allclose(loss.item(), ref_loss.item(), **LOSS_TOL)
        np.testing.assert_allclose(s.grad[:, :nv].cpu().numpy(), ref_ds.numpy(), **GRAD_TOL)
        assert _bits_zero(s.grad[:, nv:]) and q.grad is None
        # the module form with a live teacher: both gradients
        s2, q2 = s0.to(dev).requires_grad_(True), q0.to(dev).requires_grad_(True)
        loss2 = torch.clamp(w * heads.SeqKD()(s2, q2, use_blank=False, valid=(vf, shift)), -100, 100)
        loss2.backward()
        np.testing.assert_allclose(loss2.item(), ref_loss.item(), **LOSS_TOL)
        np.testing.assert_allclose(s2.grad[:, :nv].cpu().numpy(), ref_ds.numpy(), **GRAD_TOL)
        np.testing.assert_allclose(q2.grad[:, :nv].cpu().numpy(), ref_dq.numpy(), **GRAD_TOL)
        assert _bits_zero(s2.grad[:, nv:]) and _bits_zero(q2.grad[:, nv:])
        if nv == T:  # bitwise the unrestricted entry points
            s3 = s0.to(dev).requires_grad_(True)
            plain = heads.distillation_loss(s3, q0.to(dev), w)
            plain.backward()
            assert torch.equal(plain.detach().view(torch.int32), loss.detach().view(torch.int32))
            assert torch.equal(s3.grad.view(torch.int32), s.grad.view(torch.int32))


# ------------------------------------------------------------------ 3: the BiLSTM head
@pytest.fixture(scope="module")
def align():
    from scattennet_amd.alignment import AlignmentModule
    dev = _dev()
    torch.manual_seed(4)
    m = AlignmentModule(cls_num=12, input_size=8, hidden_size=8, num_layers=2, dropout=0, bidirectional=True)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(8, 3, 8, generator=g)   # (T, B, C), the reference's sequence-first input
    G = torch.randn(3, 8, 12, generator=g)  # d loss / d logits (B, T, cls)
    return m, x, G


def _run_align(m, x, G, valid=None):
    for p in m.parameters():
        p.grad = None
    xt = x.to(next(m.parameters()).device).requires_grad_(True)
    out = m(xt) if valid is None else m(xt, valid=valid)
    (out * G.to(out.device)).sum().backward()
    torch.cuda.synchronize()
    return out.detach(), xt.grad, {k: p.grad.clone() for k, p in m.named_parameters()}


@pytest.mark.parametrize("nv", [1, 5, 8])
def test_lstm_valid(align, nv):
    m, x, G = align
    dev = _dev()
    T = x.shape[0]
    Gv = G.clone()
    Gv[:, nv:] = 0  # incoming gradients beyond nv are zero, as the losses leave them
    out, dx, grads = _run_align(m, x, Gv, valid=(_valid(dev, nv, 0), 0))
    # torch.nn.LSTM + Linear on the CPU over x[:nv]
    ref = copy.deepcopy(m).cpu()
    xr = x[:nv].clone().requires_grad_(True)
    y, _ = ref.rnn(xr)
    ro = ref.gloss_layer(y).permute(1, 0, 2)  # (B, nv, cls)
    for p in ref.parameters():
        p.grad = None
    (ro * Gv[:, :nv]).sum().backward()
    np.testing.assert_allclose(out[:, :nv].cpu().numpy(), ro.detach().numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(dx[:nv].cpu().numpy(), xr.grad.numpy(), **ALIGN_TOL)
    for k, p in ref.named_parameters():
        np.testing.assert_allclose(grads[k].cpu().numpy(), p.grad.numpy(), err_msg=k, **ALIGN_TOL)
    assert _exact_zero(dx[nv:]) and bool(torch.isfinite(dx).all())
    # the package's own unpadded path at T = nv: the same kernels on the same operands
    out_u, dx_u, grads_u = _run_align(m, x[:nv], Gv[:, :nv])
    assert torch.equal(out[:, :nv].contiguous().view(torch.int32), out_u.contiguous().view(torch.int32))
    print(f"nv={nv}: dx vs unpadded rel_err {rel_err(dx[:nv], dx_u):.3g}; worst parameter gradient rel_err",
          max(rel_err(grads[k], grads_u[k]) for k in grads))
    if nv == T:
        shifted = _run_align(m, x, Gv, valid=(_valid(dev, nv, 2), 2))
        assert torch.equal(shifted[0].view(torch.int32), out.view(torch.int32))


def test_lstm_valid_reads_the_scalar_on_the_device(align):
    m, x, G = align
    dev = _dev()
    vf = _valid(dev, 8, 0)
    with torch.no_grad():
        a = m(x.to(dev), valid=(vf, 0)).clone()
        vf.fill_(5)
        b = m(x.to(dev), valid=(vf, 0))
        c = m(x[:5].to(dev))
    assert not torch.equal(a[:, :5], b[:, :5])  # the reverse direction now starts at frame 4
    assert torch.equal(b[:, :5].contiguous().view(torch.int32), c.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 4: the whole model
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


def _forward_backward(model, src):
    for p in model.parameters():
        p.grad = None
    out = model(src)
    out["total_loss"].backward()
    torch.cuda.synchronize()
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in model.named_parameters()}
    return {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in out.items()}, grads


def _truncate(src, T):
    """The fixture batch cut to T frames: lengths min(len, T), valid_len_in = len >> 1; the
    gloss lengths (3, 2, 1; clip 1 repeats a label and needs 3 frames) stay feasible."""
    lens = src["mask"].sum(1).clamp(max=T)
    out = dict(src)
    out["keypoints"], out["mask"] = src["keypoints"][:, :T].contiguous(), src["mask"][:, :T].contiguous()
    out["valid_len_in"] = (lens >> 1).to(src["valid_len_in"].dtype)
    assert bool((out["gloss_lengths"] + 1 <= out["valid_len_in"]).all())
    return out


@pytest.fixture(scope="module")
def unpadded(fx):
    """The parent-commit path: the unpadded eager run of the fixture batch (T = 26) and of its
    21-frame cut, forward + backward, computed once."""
    dev = _dev()
    model = _build(fx, dev)
    full = {k: v.to(dev) for k, v in fx["in"].items()}
    return {26: _forward_backward(model, full), 21: _forward_backward(model, _truncate(full, 21))}


def _compare(label, got, grads, want, want_grads, frames, no_grad):
    worst = {}
    for k in LOGITS:
        e = rel_err(got[k][:, :frames], want[k][:, :frames])
        worst["logits"] = max(worst.get("logits", 0.0), e)
        assert got[k][:, :frames].shape == want[k][:, :frames].shape and e < TOL, (label, k, e)
    for k in LOSSES:
        e = rel_err(got[k], want[k])
        worst["losses"] = max(worst.get("losses", 0.0), e)
        assert close(got[k], want[k], TOL), (label, k, e)
    gscale = max(float(g.abs().max()) for g in want_grads.values() if g is not None)
    for k, g in want_grads.items():
        if k in no_grad or g is None:
            continue
        assert grads[k] is not None, (label, k)
        e = rel_err(grads[k], g)
        if float(g.abs().max()) >= 1e-4 * gscale:
            worst["gradients"] = max(worst.get("gradients", 0.0), e)
        assert close(grads[k], g, TOL, gscale), (label, k, e)
    for k in no_grad:  # the alignment head: not in total_loss
        assert grads[k] is None or float(grads[k].abs().max()) == 0.0, (label, k)
    print(label, "worst rel_err", {k: f"{v:.3g}" for k, v in worst.items()})


@pytest.mark.parametrize("bucket", [28, 32, 40])
def test_padded_forward_backward_matches_the_fixture(fx, unpadded, bucket):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = S.pad_batch({k: v.to(dev) for k, v in fx["in"].items()}, bucket)
    got, grads = _forward_backward(model, src)
    assert got["fuse_coord_gloss_logits"].shape[1] == bucket // 2
    z = load_arrays("model_small")
    want = {k: torch.from_numpy(z["out." + k]) for k in LOGITS + LOSSES}
    assert want["left"].shape[1] == 13
    _compare(f"bucket {bucket} vs fixture", got, grads, want, fx["grad_param"], 13, fx["meta"]["no_grad"])
    eager, _ = unpadded[26]
    for k in ["fuse_coord_gloss_logits"] + LOSSES:
        a, b = (got[k][:, :13], eager[k]) if k in LOGITS else (got[k], eager[k])
        print(f"bucket {bucket} vs unpadded eager: {k} rel_err {rel_err(a, b):.3g}")
        assert close(a, b, TOL), (k, rel_err(a, b))


def test_padded_odd_length_matches_the_unpadded_run(fx, unpadded):
    """T = 21: frame 20 is pooled with a frame the bucket added; 21 >> 1 = 10 frames stay."""
    import scattennet_amd as S
    dev = _dev()
    want, want_grads = unpadded[21]
    for k in LOSSES:  # not a comparison of two clamped constants
        assert bool(torch.isfinite(want[k])) and 0 < float(want[k]) < 100, (k, float(want[k]))
    assert want["left"].shape[1] == 10
    model = _build(fx, dev)
    src = S.pad_batch(_truncate({k: v.to(dev) for k, v in fx["in"].items()}, 21), 32)
    assert src["valid_frames"].tolist() == [21]
    got, grads = _forward_backward(model, src)
    _compare("T 21 in bucket 32 vs unpadded", got, grads, want, want_grads, 10, fx["meta"]["no_grad"])


def _trainer(fx, dev, **kw):
    import scattennet_amd as S
    model = _build(fx, dev)
    opt = S.FusedAdam(model.parameters(), max_grad_norm=model.gradient_clip_val, **ADAM, **kw)
    return model, opt


def _batches(fx, dev):
    full = {k: v.to(dev) for k, v in fx["in"].items()}
    return {26: full, 21: _truncate(full, 21)}


def _follow(label, got, want):
    e = np.abs(np.array(got, dtype=np.float64) - np.array(want, dtype=np.float64)) / np.abs(np.array(want))
    print(label, got, "rel", e.tolist())
    assert e.max() < TOL, (label, e.tolist())


def test_one_graph_follows_the_reference_trajectory(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3)
    src = _batches(fx, dev)[26]
    losses, norms = [], []
    for _ in range(6):  # warm-up, capture, four replays
        out = bts.step(src)
        rep = S.read_report(out)
        assert rep["skipped"] is False and out["left"].shape[1] == 13
        losses.append(rep["total_loss"])
        norms.append(float(opt.grad_norm))
    assert int(opt.step_count) == 6 and bts.graphs_captured == 1
    z = load_arrays("model_small")
    _follow("bucketed loss", losses, z["train.total_loss"])
    _follow("bucketed grad norm", norms, z["train.grad_norm"])


def test_one_graph_two_lengths(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt = _trainer(fx, dev)
    twin, twin_opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3)
    b = _batches(fx, dev)
    for T in (26, 26, 21):
        out = bts.step(b[T])
        rep = S.read_report(out)
        norm = float(opt.grad_norm)
        ref = S.read_report(S.train_step(twin, twin_opt, b[T]))
        ref_norm = float(twin_opt.grad_norm)
    assert out["left"].shape[1] == 10 and bts.graphs_captured == 1 and bts._buckets[32].uses == 3
    assert int(opt.step_count) == 3 == int(twin_opt.step_count)
    _follow("third step (21 frames through the 26-frame graph) loss", [rep["total_loss"]], [ref["total_loss"]])
    _follow("third step grad norm", [norm], [ref_norm])


def test_two_buckets_follow_the_eager_twin(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt = _trainer(fx, dev, capture_slots=2)
    twin, twin_opt = _trainer(fx, dev)
    with pytest.raises(ValueError, match="capture_slots >= 2"):
        S.BucketedTrainStep(model, S.FusedAdam(model.parameters(), capture_slots=1, **ADAM), 3, (24, 32), 3)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(24, 32), label_bucket=3)
    b = _batches(fx, dev)
    losses, norms, ref_losses, ref_norms = [], [], [], []
    for T in (21, 26, 21, 26, 21, 26):
        out = bts.step(b[T])
        assert out["left"].shape[1] == T >> 1
        losses.append(S.read_report(out)["total_loss"])
        norms.append(float(opt.grad_norm))
        ref_losses.append(S.read_report(S.train_step(twin, twin_opt, b[T]))["total_loss"])
        ref_norms.append(float(twin_opt.grad_norm))
    assert bts.graphs_captured == 2 and int(opt.step_count) == 6
    assert [bts._buckets[f].uses for f in (24, 32)] == [3, 3]
    _follow("two buckets loss", losses, ref_losses)
    _follow("two buckets grad norm", norms, ref_norms)


def _state_bits(model, opt):
    ts = [p.detach() for p in model.parameters()]
    for p in model.parameters():
        st = opt.state.get(p, {})
        ts += [st[k] for k in ("exp_avg", "exp_avg_sq") if k in st]
    return [t.clone().view(torch.int32) for t in ts]


def test_nan_in_a_padded_batch_skips_the_update(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3)
    src = _batches(fx, dev)[26]
    for _ in range(2):
        S.read_report(bts.step(src))
    assert bts.graphs_captured == 1
    before = _state_bits(model, opt)
    bad = dict(src)
    bad["keypoints"] = src["keypoints"].clone()
    bad["keypoints"][1, 3, 6, 0] = float("nan")  # a valid frame of clip 1, a left-hand joint
    out = bts.step(bad)  # a replay
    assert int(opt.skipped) == 1 and int(opt.step_count) == 2
    after = _state_bits(model, opt)
    assert len(after) == len(before) > 100 and all(torch.equal(a, c) for a, c in zip(after, before))
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        S.read_report(out)
    rep = S.read_report(bts.step(src))  # the graph is fine afterwards
    assert rep["skipped"] is False and int(opt.step_count) == 3


def test_other_batch_size_falls_back_to_eager(fx):
    import scattennet_amd as S
    dev = _dev()
    model, opt = _trainer(fx, dev)
    twin, twin_opt = _trainer(fx, dev)
    bts = S.BucketedTrainStep(model, opt, batch_size=3, frame_buckets=(32,), label_bucket=3)
    full = _batches(fx, dev)[26]
    last = {k: v[:2].contiguous() for k, v in full.items()}  # an epoch's last batch: two clips
    losses, ref_losses = [], []
    for src in (full, last, full):
        out = bts.step(src)
        losses.append(S.read_report(out)["total_loss"])
        ref_losses.append(S.read_report(S.train_step(twin, twin_opt, src))["total_loss"])
    assert bts.eager_fallbacks == 1 and out["left"].shape[1] == 13 and "valid_frames" not in last
    assert bts.graphs_captured == 1 and int(opt.step_count) == 3
    _follow("fallback loss", losses, ref_losses)


# ------------------------------------------------------------ the runner alone
class _Cfg:
    cfg = {"residual_blocks": [64, 64], "max_position_embeddings": 8}  # one pooling stage


def _pooled_sums(src):
    """A step without model kernels: per clip, the keypoint sums of each pair of frames, in the
    shapes of a step's logits (B, T', 1), tokens (1, B, T'), spans (1, B, T', 2) and conf
    (1, B, T'), and the mask's frame count per clip.  Integer-valued inputs: exact in fp32."""
    kp = src["keypoints"]
    B, n = kp.shape[0], kp.shape[1] >> 1
    pooled = kp.sum((2, 3))[:, :2 * n].reshape(B, n, 2).sum(-1)
    tokens = pooled.to(torch.int32).unsqueeze(0)
    return {"left": pooled.unsqueeze(-1), "tokens": tokens, "spans": torch.stack([tokens, tokens + 1], -1),
            "conf": 0.5 * pooled.unsqueeze(0), "frames": src["mask"].sum(1)}


def _runner(dev):
    import scattennet_amd as S

    class Runner(S.BucketedStep):
        static_keys = ("keypoints", "mask", "valid_frames")
        replays = captures = 0

        def _device(self):
            return dev

        def _run(self, src):
            return _pooled_sums(src)

        def _before_replay(self):
            self.replays += 1

        def _before_capture(self):
            self.captures += 1

    return Runner(_Cfg, 2, (8, 4))


def _plain_batch(dev, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    return {"keypoints": torch.randint(-9, 10, (B, T, 5, 2), generator=g).float().to(dev),
            "mask": torch.ones(B, T, dtype=torch.int64, device=dev)}


def test_runner_alone_warms_up_captures_replays_and_trims():
    """BucketedStep with a step of a few torch ops: the protocol's counts and every return."""
    dev = _dev()
    run = _runner(dev)
    assert run.frame_buckets == (4, 8) and run.n_pool == 1 and not run.captured(4)
    captured = []
    for seed, (B, T) in enumerate([(2, 3), (2, 3), (2, 3), (2, 7), (2, 7), (1, 5)]):
        src = _plain_batch(dev, B, T, seed)
        out = run.step(src)
        captured.append(run.graphs_captured)
        want = _pooled_sums(src)
        assert set(out) == set(want) and out["left"].shape == (B, T >> 1, 1) and out["spans"].shape == (1, B, T >> 1, 2)
        for k, v in want.items():
            assert torch.equal(out[k], v), (B, T, k)
        assert out["frames"].tolist() == [T] * B  # the mask was padded with zeros
    assert captured == [0, 1, 1, 1, 2, 2]
    assert {f: run._buckets[f].uses for f in (4, 8)} == {4: 3, 8: 2}
    assert run.captured(4) and run.captured(8) and run.eager_fallbacks == 1
    assert run.captures == 2  # once per bucket
    assert run.replays == 1   # the third 3-frame batch; a capture's own first replay is not announced
    bad = _plain_batch(dev, 2, 3, 9)
    bad["mask"] = bad["mask"].to(torch.int32)
    with pytest.raises(ValueError, match="Runner: mask changed from .* to .* between batches"):
        run.step(bad)
    assert run._buckets[4].uses == 3
