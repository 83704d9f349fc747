"""The CTC loss (csrc/heads.hip: sca_ctc_loss_fwd / sca_ctc_loss_bwd) past the first trip of its
loops, at its documented limits and on labels equal to the blank, against the float64 oracle
(oracle/heads_oracle.py: ctc_compute_loss).  tests/test_heads.py stops at L = 181 and C = 1124.

  case  (B, T, C, S)        what it reaches
  a     (2, 330, 6, 150)    L = 301 and 227: the 256 boundary of the `s += 256` loops of
                            ctc_alpha_beta_kernel and of the alpha + beta copy of ctc_grad_kernel
  b     (2, 420, 5, 200)    S_b = 200 > 192: the second trip of the label threads (`j += 192`); L = 401
  c     (1, 1030, 4, 1023)  the S limit, L = 2047
  d     (2, 6, 8192, 2)     the C limit: every element of g_s[SCA_CTC_MAX_C] is initialised and read
  e     (3, 9, 7, 3)        labels equal to the blank: an empty transcript padded with 0 (tgt_len 0
                            is clamped to 1, so its one label is the blank) and a 0 inside a label row

Inputs of a-d: logits N(0, 1) float32 from an rng seeded by S, plus a boost along one even
alignment (as test_heads.test_hip_ctc_matches_oracle plants it) so that the loss stays under the
clamp at 100, which would zero every gradient; labels without adjacent repeats except one planted
in clip 1; clip 0 has S labels and clip 1 has S - S // 4; in_len = the frames the labels need +
slack (clip 0) or + 2 slack (clip 1), which is below T except in case c, whose one clip fills all
1030 frames.  Case e: logits 2 N(0, 1), rng seed 1.

Bounds.  Clips of at most 64 frames (d, e): LOSS_TOL and GRAD_TOL of tests/test_heads.py.  Longer
clips: the fp32 recursion is a running sum of T_b terms, whose worst-case rounding
tests/test_gpu_align.py derives as 4 T_b 2^-24 max(1, |nll_b|); nll_b is held to that (at least
1e-4) and every gradient element to 2e-5 + r |ref| with r = max(1e-4, 3 x that bound): alpha, beta
and nll all enter the exponent of the occupancy.  Rows t >= T_b are exactly zero.  Every element
is compared with its own bound, not in the max norm.

Torch's backward is not the reference.  On case e the oracle's nll equals
torch.nn.functional.ctc_loss in float64 for all three clips, and the oracle's gradient equals
central finite differences through torch's float64 forward to 1e-5 relative.  Torch's own CPU
backward (2.x) does not: on the clip with tgt_len 0 and label 0 it is off by about 0.1 at the
last valid frame, where it assigns the two end states of the last frame (both carry class 0
there) where it should add them.  test_oracle_gradient_is_the_finite_difference_on_blank_labels
asserts the oracle's side of that and prints torch's departure.

Measured on the MI355X, the largest ratio of an error to its bound (nll, gradient):
  a  0.014, 0.0064     b  0.0054, 0.0024     c  0.0013, 0.0013     d  0.0035, 0.0069     e  0.0065, 0.0098
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import heads_oracle as O
from tests.test_heads import GRAD_TOL, LOSS_TOL, _hip_ctc

# name -> ((B, T, C, S), boost, slack)
CASES = {
    "a_L301_L227": ((2, 330, 6, 150), 5.0, 20),
    "b_S200": ((2, 420, 5, 200), 5.0, 12),
    "c_S1023": ((1, 1030, 4, 1023), 6.0, 7),
    "d_C8192": ((2, 6, 8192, 2), 8.0, 0),
    "e_blank_labels": ((3, 9, 7, 3), None, None),
}


def _label_row(rng, C, n, repeat_at=None):
    """n labels from [1, C) with no adjacent repeat, except row[repeat_at + 1] == row[repeat_at]."""
    row = [int(rng.integers(1, C))]
    while len(row) < n:
        if repeat_at is not None and len(row) == repeat_at + 1:
            row.append(row[-1])
            continue
        c = int(rng.integers(1, C - 1))  # one of the C - 2 classes that differ from the last label
        row.append(c + (c >= row[-1]))
    return row


def _needed(row):
    return len(row) + sum(a == b for a, b in zip(row[:-1], row[1:]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(f, (loss, nll, dlogits)) of one case: the inputs as _hip_ctc takes them and the oracle's
    result, computed once and shared."""
    (B, T, C, S), boost, slack = CASES[name]
    if name == "e_blank_labels":
        x = (2.0 * np.random.default_rng(1).standard_normal((B, T, C))).astype(np.float32)
        labels = np.array([[0, 0, 0], [3, 0, 2], [4, 4, 1]], np.int32)
        tgt_len, in_len = np.array([0, 3, 3], np.int32), np.array([6, 9, 7], np.int32)
    else:
        rng = np.random.default_rng(S)
        x = rng.standard_normal((B, T, C)).astype(np.float32)
        labels = np.zeros((B, S), np.int32)
        tgt_len, in_len = np.zeros(B, np.int32), np.zeros(B, np.int32)
        for b in range(B):
            n = S if b == 0 else S - S // 4
            row = _label_row(rng, C, n, repeat_at=None if b == 0 else (n - 1) // 2)
            labels[b, :n], tgt_len[b] = row, n
            in_len[b] = _needed(row) + (1 + b) * slack
            for t in range(in_len[b]):
                x[b, t, row[min(t * n // in_len[b], n - 1)]] += boost
    f = {"logits": x, "labels": labels, "in_len": in_len, "tgt_len": tgt_len}
    return f, O.ctc_compute_loss(x, labels, in_len, tgt_len)


def _bounds(f, nll):
    """Per clip: (T_b, the bound of nll_b or None where LOSS_TOL holds, r of the gradient bound or
    None where GRAD_TOL holds)."""
    Tb, _ = O.effective_lengths(f["in_len"], f["tgt_len"])
    out = []
    for b, t in enumerate(Tb):
        if t <= 64:
            out.append((int(t), None, None))
            continue
        run = 4.0 * t * 2.0 ** -24 * max(1.0, abs(nll[b]))
        out.append((int(t), max(1e-4, run), max(1e-4, 3.0 * run)))
    return out


# ------------------------------------------------------------------ CPU: the cases themselves
@pytest.mark.parametrize("name", list(CASES))
def test_cases_are_under_the_clamp_and_have_a_gradient(name):
    f, (loss, nll, dx) = _case(name)
    (B, T, C, S), _, _ = CASES[name]
    Tb, Sb = O.effective_lengths(f["in_len"], f["tgt_len"])
    print(name, "loss", loss, "nll", nll.tolist(), "max |dlogits|", np.abs(dx).max(), "T_b", Tb.tolist(), "S_b",
          Sb.tolist())
    assert 1.0 < loss < 90.0 and np.isfinite(nll).all() and (nll > 0).all()
    assert np.abs(dx).max() >= 1e-2
    assert f["logits"].shape == (B, T, C) and f["labels"].shape == (B, S) and Sb.max() == S
    if name == "e_blank_labels":
        return
    for b in range(B):  # no adjacent repeat but the planted one, and the clip has the frames it needs
        row = f["labels"][b, :Sb[b]].tolist()
        assert min(row) >= 1 and _needed(row) - len(row) == (1 if b else 0) and _needed(row) <= Tb[b] <= T


def test_cases_reach_what_they_are_there_for():
    L = {n: (2 * O.effective_lengths(_case(n)[0]["in_len"], _case(n)[0]["tgt_len"])[1] + 1).tolist() for n in CASES}
    assert L["a_L301_L227"] == [301, 227] and L["b_S200"][0] == 401 and L["c_S1023"] == [2047]
    assert CASES["d_C8192"][0][2] == 8192 and _case("d_C8192")[0]["labels"].max() < 8192
    f = _case("e_blank_labels")[0]
    assert f["tgt_len"][0] == 0 and not f["labels"][0].any() and f["labels"][1, 1] == 0


def _torch_loss(x, f):
    """compute_loss through torch's float64 CTC forward: mean over the clips of the per-sample nll
    (every nll of case e is finite and the mean lies inside the clamp)."""
    Te, Se = O.effective_lengths(f["in_len"], f["tgt_len"])
    lp = torch.log_softmax(x, -1).clamp(-100, 0).permute(1, 0, 2)
    nll = torch.nn.functional.ctc_loss(lp, torch.tensor(f["labels"], dtype=torch.long), torch.tensor(Te),
                                       torch.tensor(Se), blank=0, reduction="none", zero_infinity=True)
    return nll.mean(), nll


def test_oracle_gradient_is_the_finite_difference_on_blank_labels():
    """Case e: the oracle's nll is torch's float64 forward, and at the last valid frame of the clip
    whose one label is the blank (tgt_len 0) the oracle's gradient is the central finite difference
    (step 1e-5) of that forward.  Torch's own backward is printed, not asserted: it departs there
    (see the module docstring), which is why the oracle is the reference."""
    f, (loss, nll, dx) = _case("e_blank_labels")
    x = torch.tensor(f["logits"], dtype=torch.float64, requires_grad=True)
    t_loss, t_nll = _torch_loss(x, f)
    np.testing.assert_allclose(nll, t_nll.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert abs(loss - float(t_loss.detach())) <= 1e-12
    t_loss.backward()
    t = int(f["in_len"][0]) - 1
    h = 1e-5
    for b, frames in ((0, [t]), (1, [0, 4, 8]), (2, [3])):
        for tt in frames:
            for c in range(f["logits"].shape[2]):
                xp, xm = x.detach().clone(), x.detach().clone()
                xp[b, tt, c] += h
                xm[b, tt, c] -= h
                fd = float(_torch_loss(xp, f)[0] - _torch_loss(xm, f)[0]) / (2 * h)
                assert abs(fd - dx[b, tt, c]) <= 1e-6 + 1e-4 * abs(dx[b, tt, c]), (b, tt, c, fd, dx[b, tt, c])
    print("torch's CPU backward minus the oracle at clip 0's last valid frame:",
          float(np.abs(x.grad[0, t].numpy() - dx[0, t]).max()), "elsewhere:",
          float(np.abs(np.delete(x.grad.numpy() - dx, t, axis=1)).max()))


def test_dimensions_past_the_limits_are_refused():
    """S = 1024 and C = 8193 are SCA_ERR_ARG from both entry points, before any GPU call: the
    pointers are stand-ins (small host buffers, never read)."""
    from scattennet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    buf = (ctypes.c_float * 16)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ERR_ARG = 1
    for fn in (lib.sca_ctc_loss_fwd, lib.sca_ctc_loss_bwd):
        fn.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 4
        fn.restype = ctypes.c_int
        for B, T, C, S in [(1, 2048, 4, 1024), (1, 2, 8193, 1), (1, 2048, 8193, 1024)]:
            assert fn(p, p, p, p, B, T, C, S, p, p, p, None) == ERR_ARG, (B, T, C, S)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_ctc_matches_oracle_past_one_pass(name):
    f, (ref_loss, ref_nll, ref_dx) = _case(name)
    loss, nll, dx = _hip_ctc(f)
    bounds = _bounds(f, ref_nll)
    worst_nll = worst_dx = 0.0
    loss_bound = 0.0
    for b, (Tb, nll_bound, r) in enumerate(bounds):
        if nll_bound is None:
            nll_bound = LOSS_TOL["atol"] + LOSS_TOL["rtol"] * abs(ref_nll[b])
            dx_bound = GRAD_TOL["atol"] + GRAD_TOL["rtol"] * np.abs(ref_dx[b, :Tb])
        else:
            dx_bound = 2e-5 + r * np.abs(ref_dx[b, :Tb])
        loss_bound += nll_bound / len(bounds)
        worst_nll = max(worst_nll, abs(nll[b] - ref_nll[b]) / nll_bound)
        worst_dx = max(worst_dx, float((np.abs(dx[b, :Tb] - ref_dx[b, :Tb]) / dx_bound).max()))
    print(f"{name}: loss {loss:.6f} (oracle {ref_loss:.6f}), error / bound: nll {worst_nll:.3g}, "
          f"dlogits {worst_dx:.3g}; T_b {[t for t, _, _ in bounds]}")
    for b, (Tb, _, _) in enumerate(bounds):
        assert not dx[b, Tb:].any(), (name, b)  # rows past the input length are exactly 0
        assert not ref_dx[b, Tb:].any()
    assert np.isfinite(dx).all()
    assert worst_nll <= 1.0, (name, nll.tolist(), ref_nll.tolist())
    # the mean of B values that are each within their bound, and the rounding of the mean itself
    assert abs(loss - ref_loss) <= loss_bound + 4 * 2.0 ** -24 * abs(ref_loss), (name, loss, ref_loss)
    assert worst_dx <= 1.0, name
