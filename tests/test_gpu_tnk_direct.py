"""The k-split weight-gradient kernel's direct-operand form (variant 46,
gemm_tnk_kernel<3, 1, true>) through ops.gemm, against a float64 product on the GPU.

Every lane of that kernel loads its own operand float4s from global memory one iteration
ahead, with no LDS image between, so the checks sit where such a loop can go wrong: one, two,
three and sixteen 64-row iterations (both ends of the prefetch and both parities of the
two-set rotation), a split-K whose last split is empty, tiles that overhang M and N, operands
that are column slices of larger NaN-filled tensors with NaN rows behind the last k row (a
stray read poisons the result), the flat grid of mixed shapes, and bitwise determinism.
"""
import pytest
import torch

TOL = 2e-5
KERNEL = "gemm_tnk_kernel<3, 1, true>"


def _rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _item(M, N, K, g, bias, pad=0, dev="cuda"):
    """dY [K, M], X [K, N], the NaN-filled outputs; pad > 0: the operands are column slices
    (offset 4, row strides M + pad and N + pad) of NaN tensors with 4 NaN rows after row K-1."""
    dY, X = torch.randn(K, M, generator=g), torch.randn(K, N, generator=g)
    if pad:
        bigY = torch.full((K + 4, M + pad), float("nan"))
        bigX = torch.full((K + 4, N + pad), float("nan"))
        bigY[:K, 4:4 + M] = dY
        bigX[:K, 4:4 + N] = X
        dY, X = bigY.to(dev)[:K, 4:4 + M], bigX.to(dev)[:K, 4:4 + N]
    else:
        dY, X = dY.to(dev), X.to(dev)
    dW = torch.full((M, N), float("nan"), device=dev)
    db = torch.full((M,), float("nan"), device=dev) if bias else None
    return dY, X, dW, db


def _probs(items, alpha=1.0, bscale=1.0):
    from scattennet_amd import ops
    out = []
    for dY, X, dW, db in items:
        K, M = dY.shape
        N = X.shape[1]
        out.append(ops._prob([ops._seg(dY, X, dY.stride(0), X.stride(0), K, alpha)], dW, M, N, N, bias_grad=db,
                             bias_grad_scale=bscale))
    return out


def _launch(items, splitk, fused, alpha=1.0, bscale=1.0):
    from scattennet_amd import _lib as L, ops
    probs = _probs(items, alpha, bscale)
    assert ops._gemm_kernel_name(L.GEMM_TN, probs, 46, splitk) == KERNEL
    ws = torch.empty(sum(splitk * (p.M * p.N + p.M) for p in probs), device="cuda") if splitk > 1 else None
    saved = ops._SPLITK_FUSED
    ops._SPLITK_FUSED = fused
    try:
        ops.gemm(L.GEMM_TN, probs, splitk=splitk, ws=ws, tile=46)
    finally:
        ops._SPLITK_FUSED = saved
    torch.cuda.synchronize()


def _check(items, alpha=1.0, bscale=1.0):
    for idx, (dY, X, dW, db) in enumerate(items):
        ref = alpha * (dY.double().t() @ X.double())
        err = _rel(dW, ref)
        print("problem", idx, tuple(dW.shape), "dW rel err", err)
        assert err < TOL, (idx, err)
        if db is not None:
            rb = alpha * bscale * dY.double().sum(0)
            err = _rel(db, rb)
            print("problem", idx, "db rel err", err)
            assert err < TOL, (idx, err)


SPLITS = [(1, False), (2, False), (2, True), (3, True)]
SHAPES = [(100, 68, True), (64, 132, False), (256, 256, True)]  # (M, N, bias)


@pytest.mark.gpu
@pytest.mark.parametrize("splitk,fused", SPLITS)
@pytest.mark.parametrize("K", [64, 128, 192, 1024])
def test_direct_operands_match_float64(K, splitk, fused):
    """Three shapes in one launch, bias on and off.  K = 128 at split-K 3 (and K = 64 at 2 or
    3) leaves the last split without an iteration; it still takes part in the combine."""
    g = torch.Generator(device="cpu").manual_seed(1000 * K + 10 * splitk + fused)
    items = [_item(M, N, K, g, bias) for M, N, bias in SHAPES]
    _launch(items, splitk, fused, alpha=2.0, bscale=0.25)
    _check(items, alpha=2.0, bscale=0.25)


@pytest.mark.gpu
@pytest.mark.parametrize("splitk,fused", SPLITS)
@pytest.mark.parametrize("K", [64, 128, 192, 1024])
def test_strided_operands_read_nothing_outside(K, splitk, fused):
    """dY and X are column slices of larger tensors: lda = M + 8, ldb = N + 8, the padding
    columns and four rows after row K-1 hold NaN."""
    g = torch.Generator(device="cpu").manual_seed(77 * K + splitk)
    items = [_item(M, N, K, g, bias, pad=8) for M, N, bias in SHAPES]
    _launch(items, splitk, fused)
    _check(items)


@pytest.mark.gpu
def test_strided_operands_same_shape_grid():
    """The same, on the (x, y, problem x split) grid of equal shapes."""
    g = torch.Generator(device="cpu").manual_seed(5)
    items = [_item(100, 132, 192, g, True, pad=12) for _ in range(3)]
    _launch(items, 2, True)
    _check(items)


@pytest.mark.gpu
@pytest.mark.parametrize("splitk,fused", SPLITS)
def test_mixed_shape_flat_grid_two_iterations(splitk, fused):
    """The mixed-shape launch of an FFN's two weight gradients and a few odd shapes, K = 128."""
    shapes = [(192, 64), (64, 192)] * 6 + [(100, 68), (68, 100), (256, 256), (40, 36)]
    g = torch.Generator(device="cpu").manual_seed(40 + splitk)
    items = [_item(M, N, 128, g, True) for M, N in shapes]
    _launch(items, splitk, fused, alpha=0.5, bscale=2.0)
    _check(items, alpha=0.5, bscale=2.0)


@pytest.mark.gpu
@pytest.mark.parametrize("K,splitk", [(1024, 3), (192, 2)])
def test_direct_operands_are_deterministic(K, splitk):
    """The same launch 10 times: every output bitwise equal."""
    g = torch.Generator(device="cpu").manual_seed(9)
    items = [_item(256, 256, K, g, True) for _ in range(6)]
    first = None
    for _ in range(10):
        for _, _, dW, db in items:
            dW.fill_(float("nan"))
            db.fill_(float("nan"))
        _launch(items, splitk, True)
        outs = [(dW.clone(), db.clone()) for _, _, dW, db in items]
        if first is None:
            first = outs
        for (a, b), (c, d) in zip(first, outs):
            assert torch.equal(a, c) and torch.equal(b, d)
    _check(items)
