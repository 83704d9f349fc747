"""The LayerNorm-fused GEMMs whose waves stage their own operand rows, through the C ABI.

gemm_ln_kernel<32, true, 1, true>'s chained passes stage the B image in wave-private rows
(wave w writes and reads rows 32w .. 32w+31) and order its writes and reads with
wavefront-scope fences only, no workgroup barrier.  A missing fence is a race: it shows up as
run-to-run differences, so every case is launched 10 times and compared bitwise, besides the
float64 check at the tolerances of tests/test_gpu_gemm_ln.py and tests/test_gpu_lnb.py.
Shapes: M = 33, 64, 100 (a partial tile, two full tiles, three tiles and a partial one) and
K = 64, 128, 192 (one to three iterations of the 64-wide main loop); sca_gemm_lnb with one and
three segments.
"""
import pytest
import torch

from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

N = 256
REPEATS = 10


def _chain_pass(L, W, bias, C, scale, aux=None):
    gelu = aux is not None
    return L.ChainPass(W.data_ptr(), W.stride(0), bias.data_ptr() if bias is not None else None, scale,
                       L.EPI_GELU if gelu else 0, C.data_ptr(), C.stride(0), aux.data_ptr() if gelu else None,
                       aux.stride(0) if gelu else 0)


@pytest.mark.parametrize("M", [33, 64, 100])
@pytest.mark.parametrize("gelu", [False, True])
@pytest.mark.parametrize("npass", [1, 2, 3])
def test_gemm_ln_chained_wave_private(npass, gelu, M):
    """sca_gemm_ln with 1-3 chained passes (pass rotation on, the library's default): float64
    parity and 10 bitwise-equal launches, K = 64, 128, 192."""
    from scattennet_amd import _lib as L, ops
    dev = torch.device("cuda:0")
    for K in (64, 128, 192):
        torch.manual_seed(1000 * M + 10 * K + npass)
        A, W = torch.randn(M, K, device=dev), torch.randn(N, K, device=dev) / K ** 0.5
        b, r = torch.randn(N, device=dev), torch.randn(M, N, device=dev)
        gam, bet = torch.randn(N, device=dev), torch.randn(N, device=dev)
        W2, b2 = torch.randn(N * npass, N, device=dev) / N ** 0.5, torch.randn(N * npass, device=dev)
        scales = [0.25 * (p + 1) for p in range(npass)]
        v, y = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
        mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
        out = torch.empty(M, N * npass, device=dev)
        aux = torch.empty(M, N * npass, device=dev) if gelu else None
        outs = [t for t in (v, y, mean, rstd, out, aux) if t is not None]
        passes = [_chain_pass(L, W2[p * N:(p + 1) * N], b2[p * N:(p + 1) * N] if p != 1 else None,
                              out[:, p * N:], scales[p], aux[:, p * N:] if gelu else None) for p in range(npass)]
        passes += [L.ChainPass()] * (3 - npass)
        prob = ops._prob([ops._seg(A, W, K, K, K)], v, M, N, N, bias=b, resid=r, ldr=N)
        ln = L.GemmLnProblem(gam.data_ptr(), bet.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                             npass, (L.ChainPass * 3)(*passes))
        first = None
        for _ in range(REPEATS):
            for t in outs:
                t.fill_(float("nan"))
            ops.gemm_ln([prob], [ln], 1e-5)
            torch.cuda.synchronize()
            got = [t.clone() for t in outs]
            if first is None:
                first = got
            assert all(torch.equal(a, c) for a, c in zip(first, got)), (K, "launches differ")
        v64 = r.double().cpu() + A.double().cpu() @ W.double().cpu().T + b.double().cpu()
        y64 = torch.nn.functional.layer_norm(v64, (N,), gam.double().cpu(), bet.double().cpu(), 1e-5)
        errs = {"v": rel_err(v.cpu(), v64), "y": rel_err(y.cpu(), y64)}
        assert errs["v"] < 1e-5 and errs["y"] < 1e-4, (K, errs)
        for p in range(npass):
            bp = b2[p * N:(p + 1) * N].double().cpu() if p != 1 else 0.0
            pre = (y64 @ W2[p * N:(p + 1) * N].double().cpu().T + bp) * scales[p]
            want = torch.nn.functional.gelu(pre) if gelu else pre
            e = rel_err(out[:, p * N:(p + 1) * N].cpu(), want)
            print("K", K, "pass", p, "rel err", e)
            assert e < 1e-4, (K, p, e)
            if gelu:
                assert rel_err(aux[:, p * N:(p + 1) * N].cpu(), pre) < 1e-4, (K, p)


@pytest.mark.parametrize("chain", ["none", "wo"])
@pytest.mark.parametrize("M", [33, 100])
@pytest.mark.parametrize("Ks", [(64,), (128,), (64, 128, 64)])
def test_gemm_lnb_segments_wave_private(Ks, M, chain):
    """sca_gemm_lnb (C = resid + sum_s A_s B_s, the LayerNorm backward of C, optionally the
    chained dout = dx Wo) on its register-staged main loop: float64 parity, 10 bitwise-equal
    launches."""
    from scattennet_amd import _lib as L, ops
    dev = torch.device("cuda:0")
    torch.manual_seed(M + sum(Ks) + len(Ks))
    segs, c64, keep = [], torch.zeros(M, N, dtype=torch.float64), []
    for K in Ks:
        A, B = torch.randn(M, K, device=dev), torch.randn(K, N, device=dev) / K ** 0.5
        keep += [A, B]
        segs.append(ops._seg(A, B, K, N, K))
        c64 += A.double().cpu() @ B.double().cpu()
    resid = torch.randn(M, N, device=dev)
    c64 += resid.double().cpu()
    x = torch.randn(M, N, device=dev) * 2 + 0.5
    gam = torch.randn(N, device=dev)
    mean = x.mean(-1)
    rstd = 1.0 / (x.var(-1, unbiased=False) + 1e-5).sqrt()
    C, dx = torch.empty(M, N, device=dev), torch.empty(M, N, device=dev)
    nblk = L.lib().sca_gemm_lnb_blocks(M)
    part = torch.empty(2 * nblk * N, device=dev)
    on = chain == "wo"
    wo = torch.randn(N, N, device=dev) / N ** 0.5
    dout = torch.empty(M, N, device=dev)
    prob = ops._prob(segs, C, M, N, N, resid=resid, ldr=N)
    lnp = L.GemmLnbProblem(x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gam.data_ptr(), dx.data_ptr(),
                           part.data_ptr(), wo.data_ptr() if on else None, dout.data_ptr() if on else None,
                           None, 0, 0)
    arr, larr = (L.GemmProblem * 1)(prob), (L.GemmLnbProblem * 1)(lnp)
    outs = [C, dx, part] + ([dout] if on else [])
    first = None
    for _ in range(REPEATS):
        for t in outs:
            t.fill_(float("nan"))
        L.check(L.lib().sca_gemm_lnb(1, arr, larr, L.stream_handle()), "sca_gemm_lnb")
        torch.cuda.synchronize()
        got = [t.clone() for t in outs]
        if first is None:
            first = got
        assert all(torch.equal(a, c) for a, c in zip(first, got)), "launches differ"
    x64 = x.double().cpu().requires_grad_(True)
    g64, b64 = gam.double().cpu().requires_grad_(True), torch.zeros(N, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(x64, (N,), g64, b64, 1e-5).backward(c64)
    assert rel_err(C.cpu(), c64) < 1e-5
    assert rel_err(dx.cpu(), x64.grad) < 1e-4
    assert rel_err(part[:nblk * N].view(nblk, N).sum(0).cpu(), g64.grad) < 1e-4
    assert rel_err(part[nblk * N:].view(nblk, N).sum(0).cpu(), b64.grad) < 1e-4
    if on:
        assert rel_err(dout.cpu(), x64.grad @ wo.double().cpu()) < 1e-4
