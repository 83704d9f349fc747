"""The fused clip + Adam update (scattennet_amd.optim.FusedAdam, csrc/optim.hip) on the GPU.

Tolerance of every parity check here (the rule of the golden-parity test): the update is
restated in float64 on the CPU (`Adam64`); stock `torch.optim.Adam` + `clip_grad_norm_` in
fp32 on the CPU has some max abs error against that restatement on the same inputs (about
5e-7 for the fixture's shapes: one ulp of max |p|); ours against the float64 restatement must
be within 4x that measured figure — the factor allows for a different but equally valid
fp32 operation order, while any formula error is of order lr = 2e-3, over 1000x larger.
"""
import math

import pytest
import torch

from tests.golden_util import load_arrays, manifest

SNAP = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


class Adam64:
    """float64 restatement of clip_grad_norm_(max_norm) + torch.optim.Adam.step() (L2 weight
    decay, optional amsgrad), one step count per parameter."""

    def __init__(self, params, group_of, hyper, amsgrad=False, max_norm=None):
        self.p = [x.detach().cpu().double().clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.vmax = [torch.zeros_like(x) for x in self.p]
        self.t = [0] * len(self.p)
        self.group_of, self.hyper, self.amsgrad, self.max_norm = group_of, hyper, amsgrad, max_norm

    def step(self, grads):
        gs = [None if g is None else g.detach().cpu().double() for g in grads]
        total = math.sqrt(sum(float((g * g).sum()) for g in gs if g is not None))
        coef = min(1.0, self.max_norm / (total + 1e-6)) if self.max_norm else 1.0
        for i, g in enumerate(gs):
            if g is None:
                continue
            h = self.hyper[self.group_of[i]]
            b1, b2 = h["betas"]
            self.t[i] += 1
            gp = coef * g + h["weight_decay"] * self.p[i]
            self.m[i] += (1 - b1) * (gp - self.m[i])
            self.v[i] = b2 * self.v[i] + (1 - b2) * gp * gp
            vh = self.v[i]
            if self.amsgrad:
                self.vmax[i] = torch.maximum(self.vmax[i], self.v[i])
                vh = self.vmax[i]
            denom = vh.sqrt() / math.sqrt(1 - b2 ** self.t[i]) + h["eps"]
            self.p[i] -= h["lr"] / (1 - b1 ** self.t[i]) * self.m[i] / denom
        return total

    def snapshot(self):
        out = {"p": [x.clone() for x in self.p], "exp_avg": [x.clone() for x in self.m],
               "exp_avg_sq": [x.clone() for x in self.v]}
        if self.amsgrad:
            out["max_exp_avg_sq"] = [x.clone() for x in self.vmax]
        return out


def _groups(params, group_of, hyper):
    return [dict(params=[p for p, g in zip(params, group_of) if g == gi], **h) for gi, h in enumerate(hyper)]


class Stock32:
    """The reference's own calls on the CPU in fp32: clip_grad_norm_ + torch.optim.Adam."""

    def __init__(self, params, group_of, hyper, amsgrad=False, max_norm=None):
        self.params = [torch.nn.Parameter(x.detach().cpu().clone()) for x in params]
        self.opt = torch.optim.Adam(_groups(self.params, group_of, hyper), amsgrad=amsgrad)
        self.max_norm, self.amsgrad = max_norm, amsgrad

    def step(self, grads):
        for p, g in zip(self.params, grads):
            p.grad = None if g is None else g.detach().cpu().clone()
        if self.max_norm:
            torch.nn.utils.clip_grad_norm_(self.params, max_norm=self.max_norm)
        self.opt.step()

    def snapshot(self):
        return _snapshot(self.params, self.opt, self.amsgrad)


def _snapshot(params, opt, amsgrad):
    names = SNAP if amsgrad else SNAP[:3]
    out = {k: [] for k in names}
    for p in params:
        st = opt.state.get(p, {})
        out["p"].append(p.detach().cpu().double())
        for k in names[1:]:
            out[k].append(st[k].detach().cpu().double() if k in st else torch.zeros(p.shape, dtype=torch.float64))
    return out


def _max_err(snap, ref):
    """max abs error over parameters and moments, and the same per quantity."""
    per = {k: max(float((a - b).abs().max()) for a, b in zip(snap[k], ref[k])) for k in ref}
    return max(per.values()), per


def _ours(dev, params, group_of, hyper, amsgrad=False, max_norm=None, make=None, **kw):
    """FusedAdam over device copies of `params` (make(i, tensor) -> the device tensor of
    parameter i, for special layouts)."""
    from scattennet_amd import FusedAdam
    make = make or (lambda i, x: x.detach().to(dev).clone())
    ps = [torch.nn.Parameter(make(i, x)) for i, x in enumerate(params)]
    return ps, FusedAdam(_groups(ps, group_of, hyper), amsgrad=amsgrad, max_grad_norm=max_norm, **kw)


def _set_grads(ps, grads, dev):
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.detach().to(dev).clone()


def _check(label, ours, stock, ref64):
    """The tolerance rule of the module docstring; returns (ours' error, stock's error)."""
    stock_err, stock_per = _max_err(stock, ref64)
    our_err, our_per = _max_err(ours, ref64)
    print(f"{label}: stock fp32 vs float64 {stock_err:.3e} {stock_per}; ours vs float64 {our_err:.3e} {our_per}; "
          f"ratio {our_err / stock_err:.3f}")
    assert stock_err > 0.0
    assert our_err <= 4.0 * stock_err, (label, our_err, stock_err, our_per, stock_per)
    return our_err, stock_err


def _fixture():
    man = manifest("manifest_optim.json")
    z = load_arrays("optim_adam_steps")
    names = man["names"]
    init = [torch.from_numpy(z[f"init.{n}"].copy()) for n in names]
    grads = [[torch.from_numpy(z[f"grad{s}.{n}"].copy()) for n in names] for s in range(1, len(man["scales"]) + 1)]
    group_of = [gi for gi, g in enumerate(man["groups"]) for _ in range(g["params"])]
    hyper = [dict(lr=g["lr"], betas=tuple(g["betas"]), eps=g["eps"], weight_decay=g["weight_decay"])
             for g in man["groups"]]
    saved = {s: {"p": [torch.from_numpy(z[f"p{s}.{n}"]).double() for n in names],
                 "exp_avg": [torch.from_numpy(z[f"exp_avg{s}.{n}"]).double() for n in names],
                 "exp_avg_sq": [torch.from_numpy(z[f"exp_avg_sq{s}.{n}"]).double() for n in names]}
             for s in man["save_after"]}
    return man, init, grads, group_of, hyper, saved, z["norms"]


# ------------------------------------------------------------------ 1: golden parity
@pytest.mark.gpu
@pytest.mark.parametrize("amsgrad", [False, True])
def test_golden_parity(amsgrad):
    """Six clipped steps from the reference fixture's initial state and gradients; parameters
    and moments after steps 1, 3 and 6 against the float64 restatement, within 4x the error
    of stock fp32 Adam (amsgrad off: the fixture's recorded values; on: torch.optim.Adam on
    the CPU, run here), and grad_norm against the norms the reference's clip returned."""
    dev = _dev()
    man, init, grads, group_of, hyper, saved, norms = _fixture()
    assert [tuple(x.shape) for x in init] == [(1,), (5,), (4097,), (258, 64), (3,), (257,), (8199,)]
    ref = Adam64(init, group_of, hyper, amsgrad, man["max_norm"])
    stock = Stock32(init, group_of, hyper, amsgrad, man["max_norm"])
    ps, opt = _ours(dev, init, group_of, hyper, amsgrad, man["max_norm"])
    ratios = []
    for s, g in enumerate(grads, start=1):
        ref.step(g)
        stock.step(g)
        _set_grads(ps, g, dev)
        opt.step()
        got_norm = float(opt.grad_norm)
        clipped = norms[s - 1] > man["max_norm"]
        print(f"step {s}: grad_norm {got_norm!r} fixture {norms[s - 1]!r} clip_coef {float(opt.clip_coef)!r}")
        assert abs(got_norm - norms[s - 1]) <= 1e-5 * norms[s - 1]
        assert (float(opt.clip_coef) < 1.0) == clipped and int(opt.step_count) == s and int(opt.skipped) == 0
        if s in man["save_after"]:
            theirs = stock.snapshot() if amsgrad else saved[s]
            our_err, stock_err = _check(f"amsgrad={amsgrad} step {s}", _snapshot(ps, opt, amsgrad), theirs,
                                        ref.snapshot())
            ratios.append(our_err / stock_err)
    print(f"parity ratio (ours / stock, worst of steps {man['save_after']}): {max(ratios):.3f}")


# ------------------------------------------------------------------ 2: shapes that can go wrong
@pytest.mark.gpu
def test_awkward_shapes_groups_and_late_gradients():
    """An unaligned parameter (a view at storage offset 1) with an unaligned gradient, sizes
    1 / 3 / 5, ten chunks over a 3-workgroup grid (the stride wraps), two groups with their own
    lr and weight decay, a parameter that never gets a gradient, and one whose first
    gradient arrives at global step 3 (its bias correction counts its own steps)."""
    from scattennet_amd.optim import CHUNK
    dev = _dev()
    gen = torch.Generator().manual_seed(5)
    sizes = [(4099,), (1,), (3,), (5,), (9 * CHUNK + 17,), (33, 7), (260,), (129,)]
    init = [torch.randn(s, generator=gen) for s in sizes]
    group_of = [0, 0, 1, 0, 1, 1, 0, 1]
    hyper = [dict(lr=2e-3, betas=(0.9, 0.998), eps=1e-8, weight_decay=2e-5),
             dict(lr=5e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=1e-2)]
    NEVER, LATE, UNALIGNED = 6, 7, 0
    steps = []
    for s in range(1, 5):
        g = [torch.randn(x.shape, generator=gen) * (10.0 if s % 2 else 1e-3) for x in init]
        g[NEVER] = None
        if s < 3:
            g[LATE] = None
        steps.append(g)

    def make(i, x):
        if i != UNALIGNED:
            return x.to(dev).clone()
        base = torch.zeros(x.numel() + 1, device=dev)
        base[1:].copy_(x.to(dev))
        return base[1:]

    ref = Adam64(init, group_of, hyper, False, 1.0)
    stock = Stock32(init, group_of, hyper, False, 1.0)
    ps, opt = _ours(dev, init, group_of, hyper, False, 1.0, make=make, max_blocks=3)
    assert ps[UNALIGNED].data_ptr() % 16 == 4 and ps[UNALIGNED].is_contiguous()
    for s, g in enumerate(steps, start=1):
        ref.step(g)
        stock.step(g)
        _set_grads(ps, g, dev)
        gbase = torch.zeros(g[UNALIGNED].numel() + 1, device=dev)  # the gradient unaligned too
        gbase[1:].copy_(g[UNALIGNED].to(dev))
        ps[UNALIGNED].grad = gbase[1:]
        opt.step()
        assert int(opt.step_count) == s
        _check(f"step {s}", _snapshot(ps, opt, False), stock.snapshot(), ref.snapshot())
    assert ps[NEVER] not in opt.state and torch.equal(ps[NEVER].detach().cpu(), init[NEVER])
    sd = opt.state_dict()
    index = {id(p): i for i, p in enumerate(q for g in opt.param_groups for q in g["params"])}
    assert index[id(ps[NEVER])] not in sd["state"]
    assert float(sd["state"][index[id(ps[LATE])]]["step"]) == 2.0  # its own count, not the global 4
    assert float(sd["state"][index[id(ps[UNALIGNED])]]["step"]) == 4.0


# ------------------------------------------------------------------ 3: reproducibility
@pytest.mark.gpu
def test_bitwise_reproducible_and_alignment_independent():
    """Two runs from the same state and gradients give bitwise-equal parameters, moments and
    grad_norm; so does a run whose parameters and gradients sit at 4-byte-aligned addresses
    (the scalar path assigns the same elements to the same threads)."""
    dev = _dev()
    man, init, grads, group_of, hyper, _, _ = _fixture()

    def run(shift):
        def put(x):
            base = torch.zeros(x.numel() + shift, device=dev)
            base[shift:].copy_(x.reshape(-1).to(dev))
            return base[shift:].view(x.shape)
        ps, opt = _ours(dev, init, group_of, hyper, True, 1.0, make=lambda i, x: put(x))
        out_norms = []
        for g in grads[:3]:
            for p, x in zip(ps, g):
                p.grad = put(x)
            opt.step()
            out_norms.append(opt.grad_norm.clone())
        snap = _snapshot(ps, opt, True)
        return [t for k in SNAP for t in snap[k]] + [n.cpu() for n in out_norms]

    a, b, c = run(0), run(0), run(1)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(torch.equal(x, y) for x, y in zip(a, c))


# ------------------------------------------------------------------ 4: skip on a non-finite loss
@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_non_finite_loss_skips_the_step(bad):
    dev = _dev()
    man, init, grads, group_of, hyper, _, _ = _fixture()

    def state_of(ps, opt):
        snap = _snapshot(ps, opt, True)
        return [t for k in SNAP for t in snap[k]]

    ps, opt = _ours(dev, init, group_of, hyper, True, 1.0)
    ps2, opt2 = _ours(dev, init, group_of, hyper, True, 1.0)  # never sees the skipped call
    fine = torch.tensor(1.25, device=dev)
    for o, q in ((opt, ps), (opt2, ps2)):
        _set_grads(q, grads[0], dev)
        o.step(loss=fine)
    before = state_of(ps, opt)
    _set_grads(ps, grads[2], dev)
    opt.step(loss=torch.tensor(bad, device=dev))
    assert int(opt.skipped) == 1 and int(opt.step_count) == 1
    assert all(torch.equal(x, y) for x, y in zip(before, state_of(ps, opt)))
    for o, q in ((opt, ps), (opt2, ps2)):
        _set_grads(q, grads[1], dev)
        o.step(loss=fine)
    assert int(opt.skipped) == 0 and int(opt.step_count) == 2 == int(opt2.step_count)
    assert all(torch.equal(x, y) for x, y in zip(state_of(ps2, opt2), state_of(ps, opt)))
    assert not any(torch.equal(x, y) for x, y in zip(before[:len(ps)], state_of(ps, opt)[:len(ps)]))


# ------------------------------------------------------------------ 5: graph capture
@pytest.mark.gpu
def test_captured_step_with_forward_and_backward():
    """Forward + backward + step() of the smoke workload's model in one hipGraph, captured
    after an eager warm-up step with p.grad = None (the gradients first exist during capture),
    replayed 3 times with the lr changed through sync_hyperparameters() between replays.
    After each replay a CPU torch.optim.Adam (with clip) advances on the replay's own
    gradients, so Adam's sensitivity at near-zero gradients stays out of the comparison."""
    from scattennet_amd import FusedAdam, ops, workloads as W
    dev = _dev()
    w = dict(B=3, T=40, K_all=27, groups=[6, 21], d=64, H=4, L=1, residual=False, maxpos=64)
    model = W.build_streams(w, dev, seed=7, init="random")
    kp, mask, gout = W.synthetic_batch(w, dev, seed=11, ragged=True)
    params = list(model.parameters())
    hyper = [dict(lr=2e-3, betas=(0.9, 0.998), eps=1e-8, weight_decay=2e-5)]
    group_of = [0] * len(params)
    ref = Adam64(params, group_of, hyper, False, 1.0)
    stock = Stock32(params, group_of, hyper, False, 1.0)
    opt = FusedAdam(params, max_grad_norm=1.0, **hyper[0])

    def fwd_bwd():
        outs = model(kp, mask)
        torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])

    def follow(label):
        torch.cuda.synchronize()
        g = [p.grad for p in params]
        assert sum(x is not None for x in g) > 10
        ref.step(g)
        stock.step(g)
        _check(label, _snapshot(params, opt, False), stock.snapshot(), ref.snapshot())

    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for p in params:
            p.grad = None
        fwd_bwd()
        opt.step()
    torch.cuda.current_stream().wait_stream(s)
    follow("eager warm-up step")
    for p in params:
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.fork_ledger_begin()
        fwd_bwd()
        ops.fork_ledger_end()
        opt.step()
    torch.cuda.synchronize()
    start = [p.detach().clone() for p in params]
    for i, lr in enumerate([2e-3, 1e-3, 3e-3]):
        for h in (opt.param_groups[0], stock.opt.param_groups[0], hyper[0]):
            h["lr"] = lr
        opt.sync_hyperparameters()
        graph.replay()
        follow(f"replay {i + 1} (lr {lr})")
    assert int(opt.step_count) == 4
    assert not any(torch.equal(a, p.detach()) for a, p in zip(start, params) if p.grad is not None)


@pytest.mark.gpu
def test_capture_needs_an_eager_step_and_a_spare_table(monkeypatch):
    """The capture-time rules of step(), driven with the capture query patched to "capturing"
    (the launches then simply run eagerly from the spare tables): no allocation under capture,
    a bounded pool of frozen tables, and sync_hyperparameters() stays outside the graph."""
    from scattennet_amd import optim
    dev = _dev()
    p = torch.nn.Parameter(torch.ones(100, device=dev))
    p.grad = torch.ones(100, device=dev)
    opt = optim.FusedAdam([p], lr=0.1)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="eager step"):
            opt.step()
    opt.step()
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        for _ in range(optim.SPARE_TABLES):
            opt.step()
        with pytest.raises(RuntimeError, match="spare table"):
            opt.step()
        opt.param_groups[0]["lr"] = 0.2
        with pytest.raises(RuntimeError, match="sync_hyperparameters"):
            opt.step()
        with pytest.raises(RuntimeError, match="outside stream capture"):
            opt.sync_hyperparameters()
    assert int(opt.step_count) == 1 + optim.SPARE_TABLES
    assert len(opt._frozen) == optim.SPARE_TABLES and all(t.host.is_pinned() for t in opt._frozen)


# ------------------------------------------------------------------ 6: data-parallel layout
@pytest.mark.gpu
def test_step_reads_gradient_bucket_slots():
    """With GradBuckets the gradients are views into the reducer's flat buffer: after the
    planning backward and one more backward, step() reads the slots."""
    from scattennet_amd import FusedAdam, ops, workloads as W
    from scattennet_amd.dp import GradBuckets
    dev = _dev()
    w = dict(B=3, T=40, K_all=27, groups=[6, 21], d=64, H=4, L=1, residual=False, maxpos=64)
    model = W.build_streams(w, dev, seed=7, init="random")
    kp, mask, gout = W.synthetic_batch(w, dev, seed=11, ragged=True)
    params = list(model.parameters())
    hyper = [dict(lr=2e-3, betas=(0.9, 0.998), eps=1e-8, weight_decay=2e-5)]
    group_of = [0] * len(params)
    ref = Adam64(params, group_of, hyper, False, 1.0)
    stock = Stock32(params, group_of, hyper, False, 1.0)
    opt = FusedAdam(params, max_grad_norm=1.0, **hyper[0])
    red = GradBuckets(params, world=1)
    try:
        for _ in range(2):  # the planning backward, then a bucketed one
            for p in params:
                p.grad = None
            outs = model(kp, mask)
            torch.autograd.backward(outs, [gout[g] for g in range(len(outs))])
        assert red.plan is not None and len(red.slot) > 10
        lo, hi = red.flat.data_ptr(), red.flat.data_ptr() + 4 * red.flat.numel()
        assert all(lo <= params[i].grad.data_ptr() < hi for i in red.slot)
        opt.step()
        torch.cuda.synchronize()
        g = [p.grad for p in params]
        ref.step(g)
        stock.step(g)
        _check("bucketed gradients", _snapshot(params, opt, False), stock.snapshot(), ref.snapshot())
    finally:
        red.close()
        ops.set_grad_sink(None)


# ------------------------------------------------------------------ 7: checkpoints
@pytest.mark.gpu
@pytest.mark.parametrize("amsgrad", [False, True])
def test_checkpoint_round_trip_with_torch_adam(amsgrad):
    """state_dict() after 2 steps loads into torch.optim.Adam and a torch.optim.Adam
    checkpoint loads into FusedAdam; a third step from either side agrees with the float64
    restatement of all three steps within the parity tolerance."""
    dev = _dev()
    man, init, grads, group_of, hyper, _, _ = _fixture()
    ref = Adam64(init, group_of, hyper, amsgrad, 1.0)
    stock = Stock32(init, group_of, hyper, amsgrad, 1.0)
    ps, opt = _ours(dev, init, group_of, hyper, amsgrad, 1.0)
    for g in grads[:2]:
        ref.step(g)
        stock.step(g)
        _set_grads(ps, g, dev)
        opt.step()
    ours_sd, stock_sd = opt.state_dict(), stock.opt.state_dict()
    assert ours_sd["param_groups"] == stock_sd["param_groups"]
    assert set(ours_sd["state"]) == set(stock_sd["state"])
    for k, st in ours_sd["state"].items():
        assert set(st) == set(stock_sd["state"][k]) and float(st["step"]) == 2.0

    # ours -> torch.optim.Adam (CPU copies of our parameters)
    taker = Stock32([p.detach() for p in ps], group_of, hyper, amsgrad, 1.0)
    taker.opt.load_state_dict(ours_sd)
    # torch.optim.Adam -> ours (device copies of its parameters)
    ps2, opt2 = _ours(dev, [p.detach() for p in stock.params], group_of, hyper, amsgrad, 1.0)
    opt2.load_state_dict(stock_sd)

    ref.step(grads[2])
    stock.step(grads[2])
    taker.step(grads[2])
    _set_grads(ps2, grads[2], dev)
    opt2.step()
    assert int(opt2.step_count) == 3
    stock_err, _ = _max_err(stock.snapshot(), ref.snapshot())
    for label, snap in (("ours -> torch", taker.snapshot()), ("torch -> ours", _snapshot(ps2, opt2, amsgrad))):
        err, per = _max_err(snap, ref.snapshot())
        print(f"{label}: {err:.3e} {per}; stock {stock_err:.3e}; ratio {err / stock_err:.3f}")
        assert err <= 4.0 * stock_err, (label, err, stock_err)
    assert all(float(st["step"]) == 3.0 for st in opt2.state_dict()["state"].values())


# ------------------------------------------------------------------ 8: stand-alone clip
@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", [1.0, 1e9])
def test_stand_alone_clip_grad_norm(max_norm):
    """clip_grad_norm_ against torch's on copies.  The norm within 1e-5 relative (a fixed-order
    fp32 sum of this length: worst case about 2e-6).  Each clipped gradient within 4 * 2^-24
    relative of g * max_norm / (norm + 1e-6) evaluated in float64 from the norm WE returned:
    three fp32 roundings remain (add, divide, multiply), 2^-24 relative each; against torch's
    own clipped gradients the two norms' 1e-5 bound applies twice.  An idle clip leaves the
    bits alone."""
    from scattennet_amd import clip_grad_norm_
    dev = _dev()
    gen = torch.Generator().manual_seed(9)
    shapes = [(1,), (3,), (5,), (257,), (4097,), (258, 64), (8199,), (2 * 8192 + 1,)]
    cpu = [torch.nn.Parameter(torch.zeros(s)) for s in shapes] + [torch.nn.Parameter(torch.zeros(4))]
    gpu = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes] + \
        [torch.nn.Parameter(torch.zeros(4, device=dev))]
    for i, (a, b) in enumerate(zip(cpu[:-1], gpu[:-1])):  # the last one has no gradient
        a.grad = torch.randn(a.shape, generator=gen)
        if i == 4:  # an unaligned gradient
            base = torch.zeros(a.numel() + 1, device=dev)
            base[1:].copy_(a.grad.to(dev))
            b.grad = base[1:]
        else:
            b.grad = a.grad.to(dev).clone()
    before = [b.grad.clone() for b in gpu[:-1]]
    want = torch.nn.utils.clip_grad_norm_(cpu, max_norm=max_norm)
    got = clip_grad_norm_(gpu, max_norm)
    assert got.is_cuda and got.dim() == 0 and gpu[-1].grad is None
    print(f"norm ours {float(got)!r} torch {float(want)!r}")
    assert abs(float(got) - float(want)) <= 1e-5 * float(want)
    coef = min(1.0, max_norm / (float(got) + 1e-6))
    for a, b, b0 in zip(cpu[:-1], gpu[:-1], before):
        if max_norm > float(want):
            assert torch.equal(b.grad, b0)
        want_g = b0.double().cpu() * coef  # from OUR norm: what remains is add, divide, multiply
        err = float((b.grad.cpu().double() - want_g).abs().max())
        assert err <= 4 * 2.0 ** -24 * float(want_g.abs().max()), (tuple(a.shape), err)
        assert float((b.grad.cpu() - a.grad).abs().max()) <= 2e-5 * float(a.grad.abs().max())  # and torch's
