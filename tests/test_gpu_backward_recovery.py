"""A backward that raises before its final callbacks (a user hook throwing at its very end, after
every weight-gradient section) must not poison the next one: the side-stream join and the
deferred LayerNorm affine reductions belong to the autograd graph task's state
(ops._backward), so the next backward queues its own join / flush and drops the failed
one's pending reductions.  Checked bitwise against a clean backward (the kernels are
deterministic)."""
import pytest
import torch

from scattennet_amd import workloads as W

pytestmark = pytest.mark.gpu


def test_backward_after_a_raised_backward():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    w = dict(W.WORKLOADS["cfg2"], B=2)
    model = W.build_streams(w, dev, seed=3, init="random")
    kp, mask, gout = W.synthetic_batch(w, dev, seed=5, ragged=True)

    def run(x):
        outs = model(x, mask)
        torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])

    run(kp)
    torch.cuda.synchronize()
    ref = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
    assert ref
    model.zero_grad(set_to_none=True)

    kp_bad = kp.clone().requires_grad_(True)  # its gradient is the backward's last product

    def boom(_):
        raise RuntimeError("boom")

    kp_bad.register_hook(boom)
    with pytest.raises(RuntimeError, match="boom"):
        run(kp_bad)
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)

    run(kp)
    torch.cuda.synchronize()
    got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(ref)
    for n, g in got.items():
        assert torch.equal(g, ref[n]), n


def _grads(model):
    return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}


def _setup(seed=3):
    dev = torch.device("cuda:0")
    w = dict(W.WORKLOADS["cfg2"], B=2)
    model = W.build_streams(w, dev, seed=seed, init="random")
    kp, mask, gout = W.synthetic_batch(w, dev, seed=5, ragged=True)
    return model, kp, mask, gout


def test_stale_reductions_are_dropped_when_the_next_backward_defers_nothing():
    """After a raised backward, a flush outside that backward (or from a backward that defers
    nothing, e.g. accumulating into held .grad) launches none of its pending reductions."""
    from scattennet_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, kp, mask, gout = _setup()

    def run(x):
        outs = model(x, mask)
        torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])

    run(kp)
    torch.cuda.synchronize()
    ref = _grads(model)
    kp_bad = kp.clone().requires_grad_(True)
    kp_bad.register_hook(lambda _: (_ for _ in ()).throw(RuntimeError("boom")))
    model.zero_grad(set_to_none=True)
    with pytest.raises(RuntimeError, match="boom"):
        run(kp_bad)
    torch.cuda.synchronize()
    for n, p in model.named_parameters():  # the void gradients of the raised backward, held on
        if p.grad is not None:             # purpose: a stale reduction would write into them
            p.grad = ref[n].clone()
    held = _grads(model)
    ops.flush_deferred_affine()  # outside any backward: must drop, not launch
    assert not ops._bwd.affine and not ops._bwd.held and not ops._bwd.joins and not ops._bwd.flush_queued
    torch.cuda.synchronize()
    for n, g in _grads(model).items():
        assert torch.equal(g, held[n]), n
    run(kp)  # accumulates into the held gradients: nothing deferred
    torch.cuda.synchronize()
    got = _grads(model)
    assert set(got) == set(ref)
    for n, g in got.items():  # parameters the raised backward never reached start from None
        assert torch.equal(g, held[n] + ref[n] if n in held else ref[n]), n


def _reference_grads(model, run):
    """The same backward with every gradient written in place on the calling stream (no side
    stream, no deferred reductions) — checked: the fork ledger sees no fork or join, and
    nothing is left held or deferred."""
    from scattennet_amd import ops
    side, defer = ops._WGRAD_SIDE, ops._AFFINE_DEFER
    ops._WGRAD_SIDE, ops._AFFINE_DEFER = False, False
    try:
        model.zero_grad(set_to_none=True)
        ledger = ops.fork_ledger_begin()
        try:
            out = run()
        finally:
            ops.fork_ledger_end()
        assert ledger.seq == 0 and not ledger.last_fork and not ledger.last_join
        assert not ops._bwd.held and not ops._bwd.affine
        torch.cuda.synchronize()
        return _grads(model), out
    finally:
        ops._WGRAD_SIDE, ops._AFFINE_DEFER = side, defer
        model.zero_grad(set_to_none=True)


def _churn(dev):
    """Allocations that would take over any gradient block freed too early."""
    return [torch.full((1 << 16,), 7.0, device=dev) for _ in range(64)]


def test_frozen_layernorm_gradients_match_the_in_place_path():
    """A frozen LayerNorm (requires_grad False: autograd drops its dgamma / dbeta) must not
    leave a deferred reduction writing into freed memory; every other gradient bitwise equal to
    the in-place path."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, kp, mask, gout = _setup()
    frozen = [m for n, m in model.named_modules() if n.endswith("attn_layer_norm")][:3]
    for m in frozen:
        m.weight.requires_grad_(False)
        m.bias.requires_grad_(False)

    def run():
        outs = model(kp, mask)
        keep = _churn(kp.device)
        torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])
        return keep

    ref, _ = _reference_grads(model, run)
    keep = run()
    torch.cuda.synchronize()
    got = _grads(model)
    assert set(got) == set(ref)
    for n, g in got.items():
        assert torch.equal(g, ref[n]), n
    for t in keep:
        assert bool((t == 7.0).all())
    for m in frozen:
        assert m.weight.grad is None and m.bias.grad is None


def test_input_only_autograd_grad_leaves_parameters_alone():
    """torch.autograd.grad w.r.t. the keypoints only: no parameter gradient is kept, the input
    gradient equals the in-place path's, and no live tensor is overwritten."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, kp, mask, gout = _setup()
    x = kp.clone().requires_grad_(True)

    def run():
        outs = model(x, mask)
        keep = _churn(kp.device)
        (g,) = torch.autograd.grad(outs, [x], [gout[i] for i in range(len(outs))])
        return g, keep

    _, (ref, _) = _reference_grads(model, run)
    got, keep = run()
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    assert all(p.grad is None for p in model.parameters())
    for t in keep:
        assert bool((t == 7.0).all())


def test_a_block_used_twice_accumulates_complete_gradients():
    """The same attention block applied twice in one graph: autograd adds the second weight
    gradient into the first on the calling stream, so the first (side stream) must be complete
    by then."""
    import scattennet_amd as S
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    cfg = W.model_cfg(256, 16, 1, maxpos=64)
    blk = S.CoordinateAttention(cfg, "self_attn").to(dev)
    x = torch.randn(4, 64, 256, device=dev)
    mask = S.key_padding_mask(torch.ones(4, 64, dtype=torch.long, device=dev))
    g = torch.randn(4, 64, 256, device=dev)

    def run():
        y = blk(blk(x, mask), mask)
        y.backward(g)

    ref, _ = _reference_grads(blk, run)
    blk.zero_grad(set_to_none=True)
    run()
    torch.cuda.synchronize()
    got = _grads(blk)
    assert set(got) == set(ref)
    for n, t in got.items():
        assert torch.allclose(t, ref[n], rtol=0, atol=1e-6 * float(ref[n].abs().max())), n


@pytest.mark.parametrize("hold", [1, 5, 10, 19, 40])
def test_held_weight_gradient_sections_match_the_in_place_path(hold, monkeypatch):
    """ops.weight_grads holding the first `hold` SCA sections of a backward and issuing them
    together (equal shapes across sections in shared launches) at the last one's fork — or at
    the join when the backward has fewer sections: every gradient bitwise equal to the in-place
    path's (same kernels, same reduction order per problem)."""
    from scattennet_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, kp, mask, gout = _setup(seed=7)
    monkeypatch.setattr(ops, "_WGRAD_HOLD_FRAC", float(hold))

    def run():
        outs = model(kp, mask)
        torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])

    ref, _ = _reference_grads(model, run)
    for _ in range(2):  # the second backward holds by the first's section count too
        model.zero_grad(set_to_none=True)
        run()
        torch.cuda.synchronize()
        got = _grads(model)
        assert set(got) == set(ref)
        for n, g in got.items():
            assert torch.equal(g, ref[n]), n
    assert not ops._bwd.held


def test_a_backward_that_begins_elsewhere_holds_nothing_and_the_next_one_holds():
    """Only a backward whose first weight-gradient section is holdable holds.  One that begins
    with a plain linear head forks every section, and still counts its holdable sections: the
    next backward, beginning with an SCA block, holds the first half of that count.  Both
    bitwise equal to the in-place path."""
    from scattennet_amd import ops
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    model, kp, mask, gout = _setup(seed=7)
    G, d = len(gout), gout[0].shape[-1]
    torch.manual_seed(13)
    head = torch.nn.ModuleList([torch.nn.Linear(d, d) for _ in range(G)]).to(kp.device)
    both = torch.nn.ModuleList([model, head])

    def run_headed():
        outs = ops.LinearResidual.apply(G, False, *model(kp, mask), *[h.weight for h in head],
                                        *[h.bias for h in head])
        torch.autograd.backward(outs, [gout[g] for g in range(G)])

    def run_plain():
        outs = model(kp, mask)
        torch.autograd.backward(outs, [gout[g] for g in range(G)])

    assert 0 < ops._WGRAD_HOLD_FRAC < 1  # the default: a fraction of the previous backward's sections
    ref_headed, _ = _reference_grads(both, run_headed)
    ref_plain, _ = _reference_grads(model, run_plain)

    def check(module, ref):
        torch.cuda.synchronize()
        got = _grads(module)
        assert set(got) == set(ref)
        for n, g in got.items():
            assert torch.equal(g, ref[n]), n
        module.zero_grad(set_to_none=True)

    run_headed()
    check(both, ref_headed)
    total = ops._bwd.count
    assert total > 0 and ops._bwd.hold == 0 and ops._bwd.n_held == 0
    run_plain()
    check(model, ref_plain)
    assert ops._bwd.last_total == total and ops._bwd.count == total
    assert ops._bwd.hold == ops._bwd.n_held == int(round(ops._WGRAD_HOLD_FRAC * total)) > 0
    assert not ops._bwd.held
