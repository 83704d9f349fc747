"""The MWER loss, rescoring and MBR on hand-built lists up to the 128-token limit of the WER kernel
(csrc/mwer.hip, csrc/decode.hip), against the float64 restatements of tests/mwer_ref.py and
tests/nbest_ref.py.  The shared n-best cases stop at entries of about 104 tokens; here
mwer_alpha_beta's five states per lane (lane + 64 k, k < MW_K = 5) are all used, the `s += 256`
and `j += 192` loops of mwer_grad_kernel take a second trip, and a reference longer than the
list's width sets the workspace stride (Hm = R > H).

B = 2, T = 128, C = 9, N = 5, in_len = [128, 112], rng seed 3.  The references are label rows
without adjacent repeats, of 128 tokens (clip 0) and 97 tokens (clip 1); the logits are N(0, 1)
plus 3.0 along each reference's even alignment.  Lists:
  clip 0   the reference itself (128 tokens in 128 frames: L = 257, no slack, every state forced;
           k = 4 holds exactly one state), one substitution at position 70, the reference without
           token 100, the reference without tokens 30-31, its first 64 tokens
  clip 1   the reference without token 50 (L = 193), the reference itself (L = 195), token 10 set
           equal to token 9 (a repeat), the reference plus one appended token, its first 95 tokens
           (L = 191): the 192 boundary between k = 2 and k = 3 is crossed from both sides
Modes: `plain`; `table` (mwer_ref.random_lm(9) with this file's LM_WEIGHT and LENGTH_BONUS);
`reference` with the list's width cut to H = 100 under R = 128: entry e of clip 0 keeps its first
100 - e tokens (entry 0 is then the reference's first 100 tokens, and the entries stay distinct),
and clip 1 loses its copy of the reference, so that the reference slot is valid in both clips.
There clip 0's reference slot takes the whole posterior (every entry lacks 28 tokens or more), so
clip 0's gradient is rounding alone (1e-16 in float64) and its per-clip check says little; clip 1
carries that mode (posteriors 0.316, 0.166 and the reference slot's 0.518, max |dlogits| 0.0898), and
its workspace rows lie behind clip 0's six slots of stride 2 * 128 + 1.

Asserted: tests/mwer_gpu.py's _assert_parity under the project's TOL = 1e-3, dlogits also per clip
(rel_err is a max norm over the whole tensor), rows t >= in_len[b] exactly zero, the captured
forward and backward bitwise the eager call, and on the `plain` lists rescore_nbest_device and
mbr_select_device against nbest_ref's rescore and mbr (loss, order and best equal; total, posterior
and risk within TOL max(1, |ref|)).

Restated values (CPU, float64): RESTATED below.  Measured on the MI355X, _assert_parity's rel_err
figures (loglik, posterior, risk, loss, dlogits; then dlogits per clip):
  plain      4.7e-8, 3.1e-6, 2.5e-6, 2.1e-7, 1.2e-5;  1.1e-5, 1.2e-5
  table      4.7e-8, 5.0e-6, 3.4e-6, 2.9e-7, 1.0e-5;  1.2e-5, 1.0e-5
  reference  1.6e-7, 8.5e-7, 9.3e-7, 0,      1.2e-5;  4.8e-15 (against the floor of rel_err), 1.2e-5
Rescoring and MBR of the `plain` lists: largest error 8.0e-6 of max(1, |ref|).
"""
import functools

import numpy as np
import pytest
import torch

from tests import mwer_ref as M
from tests import nbest_ref as NR
from tests.golden_util import rel_err
from tests.mwer_gpu import TOL, _assert_parity, _bits, _dev, _lm, _nbest, _run
from tests.test_gpu_ctc_long import _label_row

MIN_GAP = 1e-4
B, T, C, N = 2, 128, 9, 5
IN_LEN = [128, 112]
SEED = 3
BOOST = 3.0
H_CUT = 100  # the list's width in `reference` mode; R = 128
# The `table` mode's weights.  mwer_ref's (0.7, 0.3) cost about 2.4 log units per token (the table's
# mean entry is -3.8), which over entries 64 tokens apart hands the whole posterior to the shortest
# entry; these are nearly length-neutral (0.1 x -3.8 + 0.4), so the prior reorders the close
# entries and every clip keeps two slots that count.
LM_WEIGHT, LENGTH_BONUS = 0.1, 0.4
MODES = ("plain", "table", "reference")

# plain mode, float64 restatement: loglik / posterior / errors of entries 0-4
RESTATED = {
    0: ([-71.5, -76.1, -71.7, -75.9, -195.1], [0.513, 0.013, 0.458, 0.016, 0.0], [0, 1, 1, 2, 64]),
    1: ([-63.3, -62.7, -72.5, -80.9, -64.1], [0.316, 0.518, 0.0, 0.0, 0.166], [1, 0, 1, 1, 2]),
}  # max |dlogits| 0.0912 (clip 0) and 0.0898 (clip 1); `table`: 0.0917 and 0.1218


def _other(*near):
    """The smallest class in [1, C) that is none of `near`."""
    return next(c for c in range(1, C) if c not in near)


@functools.lru_cache(maxsize=None)
def _inputs(mode="plain"):
    """(logits (B, T, C) float32, in_len, lists, refs, H) of a mode."""
    rng = np.random.default_rng(SEED)
    refs = [_label_row(rng, C, 128), _label_row(rng, C, 97)]
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    for b, r in enumerate(refs):
        for t in range(IN_LEN[b]):
            x[b, t, r[min(t * len(r) // IN_LEN[b], len(r) - 1)]] += BOOST
    r0, r1 = refs
    sub = r0[:70] + [_other(r0[69], r0[70], r0[71])] + r0[71:]
    lists = [[r0, sub, r0[:100] + r0[101:], r0[:30] + r0[32:], r0[:64]],
             [r1[:50] + r1[51:], r1, r1[:10] + [r1[9]] + r1[11:], r1 + [_other(r1[-1])], r1[:95]]]
    if mode != "reference":
        return x, IN_LEN, lists, refs, T
    cut = [[h[:H_CUT - e] for e, h in enumerate(lists[0])], [h for h in lists[1] if h != r1]]
    return x, IN_LEN, cut, refs, H_CUT


def _kw(mode):
    if mode == "table":
        return dict(lm=M.random_lm(C), lm_weight=LM_WEIGHT, length_bonus=LENGTH_BONUS)
    return dict(reference=True) if mode == "reference" else {}


@functools.lru_cache(maxsize=None)
def _want(mode):
    """The restatement of a mode, computed once and shared."""
    x, in_len, lists, refs, _ = _inputs(mode)
    kw = dict(_kw(mode))
    with_ref = kw.pop("reference", False)
    return M.mwer(x, in_len, lists, refs, M.POSTERIOR_SCALE, n_max=N, with_ref=with_ref, **kw)


@functools.lru_cache(maxsize=None)
def _rescored():
    """nbest_ref's rescoring and MBR of the `plain` lists, scored by the restated likelihoods as
    float32 holds them: per clip (entries, total, posterior, order, loss, risk, best)."""
    _, _, lists, _, _ = _inputs()
    scores = _want("plain")["loglik"].astype(np.float32)
    out = []
    for b in range(B):
        entries = [(h, float(scores[b, n])) for n, h in enumerate(lists[b])]
        total, post, order = NR.rescore(entries, NR.random_lm(C), NR.LM_WEIGHT, NR.LENGTH_BONUS, NR.POSTERIOR_SCALE)
        loss, risk, best = NR.mbr(entries, post)
        out.append((entries, total, post, order, loss, risk, best))
    return scores, out


# ------------------------------------------------------------------ CPU: the inputs
def test_lists_are_what_the_docstring_says():
    _, _, lists, refs, _ = _inputs()
    assert [len(r) for r in refs] == [128, 97] and all(M.fits(r, Tb) for r, Tb in zip(refs, IN_LEN))
    assert all(a != b for r in refs for a, b in zip(r[:-1], r[1:])) and all(1 <= c < C for r in refs for c in r)
    assert [[2 * len(h) + 1 for h in clip] for clip in lists] == [[257, 257, 255, 253, 129], [193, 195, 195, 197, 191]]
    assert all(M.fits(h, IN_LEN[b]) for b, clip in enumerate(lists) for h in clip)
    assert not M.fits(lists[0][0] + [1], IN_LEN[0])  # clip 0's reference has no slack
    assert lists[1][2][10] == lists[1][2][9]
    for clip in lists + _inputs("reference")[2]:
        assert len(set(map(tuple, clip))) == len(clip)
    _, _, cut, _, H = _inputs("reference")
    assert H == H_CUT and [len(h) for h in cut[0]] == [100, 99, 98, 97, 64] and cut[0][0] == refs[0][:100]
    assert len(cut[1]) == 4 and max(len(h) for h in cut[1]) == 98 <= H and max(len(r) for r in refs) == 128 > H


@pytest.mark.parametrize("mode", MODES)
def test_restatement_is_informative(mode):
    """Every clip has at least two slots with posterior >= 0.04 and max |dlogits| >= 1e-2 (in
    `reference` mode: clip 1, see the module docstring), and the closed form equals autograd."""
    x, in_len, lists, refs, _ = _inputs(mode)
    want = _want(mode)
    for b in range(B):
        print(mode, "clip", b, "loglik", np.round(want["loglik"][b], 1).tolist(), "posterior",
              np.round(want["posterior"][b], 3).tolist(), "errors", want["errors"][b].tolist(), "max |dlogits|",
              float(np.abs(want["dlogits"][b]).max()))
    informative = [1] if mode == "reference" else [0, 1]
    for b in informative:
        assert (want["posterior"][b] >= 0.04).sum() >= 2, (mode, b)
        assert np.abs(want["dlogits"][b]).max() >= 1e-2, (mode, b)
        assert not want["dlogits"][b, in_len[b]:].any()
    for b, clip in enumerate(lists):  # every entry fits; the slots past count do not exist
        assert np.isfinite(want["loglik"][b, :len(clip)]).all() and np.isneginf(want["loglik"][b, len(clip):N]).all()
    if mode == "reference":
        assert want["ref_valid"].tolist() == [1, 1] and np.isfinite(want["loglik"][:, N]).all()
        assert want["posterior"][0, N] > 1.0 - 1e-9 and want["posterior"][1, N] >= 0.04
    if mode == "plain":
        for b, (ll, post, errs) in RESTATED.items():  # the recorded values are the restatement's
            assert np.round(want["loglik"][b], 1).tolist() == ll and np.round(want["posterior"][b], 3).tolist() == post
            assert want["errors"][b].tolist() == errs
    kw = dict(_kw(mode))
    with_ref = kw.pop("reference", False)
    got = M.analytic_grad(x, in_len, lists, refs, M.POSTERIOR_SCALE, with_ref=with_ref, **kw)
    assert np.abs(got - want["dlogits"]).max() < 1e-9


def test_rescored_plain_lists_are_away_from_ties():
    """The two smallest restated risks and the neighbouring totals are at least MIN_GAP apart."""
    _, clips = _rescored()
    for b, (entries, total, post, order, loss, risk, best) in enumerate(clips):
        gaps = {"total": NR.adjacent_gap(total[order]), "risk": NR.adjacent_gap(-np.sort(risk)[:2])}
        print("clip", b, "total", np.round(total, 2).tolist(), "posterior", np.round(post, 3).tolist(), "risk",
              np.round(risk, 3).tolist(), "best", best, "order", order, gaps)
        assert min(gaps.values()) >= MIN_GAP, (b, gaps)
    assert clips[0][4][4, 0] == 64  # the 64-token entry against the 128-token one


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_kernels_against_the_restatement(mode):
    x, in_len, lists, refs, H = _inputs(mode)
    want = _want(mode)
    loss, det, dx = _run(x, in_len, lists, refs, N, H, _dev(), M.POSTERIOR_SCALE, **_kw(mode))
    with_ref = mode == "reference"
    assert det["loglik"].shape == (B, N + with_ref) and ("ref_valid" in det) == with_ref and loss.dim() == 0
    _assert_parity(f"long lists, {mode}", loss, det, dx, want)
    per_clip = [rel_err(dx[b], torch.from_numpy(want["dlogits"][b])) for b in range(B)]
    print(f"long lists, {mode}: dlogits per clip", ["%.3g" % v for v in per_clip], "max |dlogits_ref| per clip",
          ["%.3g" % np.abs(want["dlogits"][b]).max() for b in range(B)])
    for b in range(B):
        assert per_clip[b] < TOL, (mode, b, per_clip[b])
        assert not dx[b, in_len[b]:].any(), (mode, b)  # rows past in_len are written as zeros
        n = len(lists[b])  # the slots past count: no posterior, no likelihood
        assert not det["posterior"][b, n:N].any() and np.isneginf(det["loglik"][b, n:N].numpy()).all(), (mode, b)
    assert torch.isfinite(dx).all()


@pytest.mark.gpu
def test_captured_forward_and_backward_replay_bitwise():
    """`reference` mode's inputs with the table on: the captured call replayed on the same inputs is
    bitwise the eager call."""
    import scattennet_amd as S
    dev = _dev()
    logits, in_len, lists, refs, H = _inputs("reference")
    x = torch.from_numpy(logits).to(dev).requires_grad_(True)
    il = torch.tensor(in_len, dtype=torch.int32, device=dev)
    ref, ref_len = (torch.from_numpy(a).to(dev) for a in M.pack_refs(refs))
    nb = _nbest(lists, N, H, dev)
    lm = _lm(M.random_lm(C), dev)

    def chain():
        x.grad = None
        loss, det = S.mwer_loss(x, il, ref, ref_len, nbest=nb, posterior_scale=M.POSTERIOR_SCALE, return_details=True,
                                reference=True, lm=lm, lm_weight=LM_WEIGHT, length_bonus=LENGTH_BONUS)
        loss.backward()
        return [loss.detach(), det["loglik"], det["posterior"], det["errors"], det["ref_valid"], det["risk"], x.grad]

    eager = [t.clone() for t in chain()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(outs, eager)):
            assert torch.equal(_bits(a), _bits(b)), (rep, i)
    assert eager[6].abs().max() > 0 and eager[4].tolist() == [1, 1]


@pytest.mark.gpu
def test_rescoring_and_mbr_of_the_plain_lists():
    import scattennet_amd as S
    dev = _dev()
    _, _, lists, _, _ = _inputs()
    scores, clips = _rescored()
    nb = _nbest(lists, N, T, dev)
    nb = S.NBest(nb.tokens, nb.lengths, torch.from_numpy(scores).to(dev), nb.count)
    lm = S.BigramLM(NR.random_lm(C), device=dev)
    total, post, order = S.rescore_nbest_device(nb, lm, NR.LM_WEIGHT, NR.LENGTH_BONUS, NR.POSTERIOR_SCALE)
    best, risk, loss = S.mbr_select_device(nb, post)
    total, post, order, best, risk, loss = (t.cpu().numpy() for t in (total, post, order, best, risk, loss))
    worst = 0.0
    for b, (entries, w_total, w_post, w_order, w_loss, w_risk, w_best) in enumerate(clips):
        assert loss[b].tolist() == w_loss.tolist() and order[b].tolist() == w_order and int(best[b]) == w_best, b
        for got, ref in ((total[b], w_total), (post[b], w_post), (risk[b], w_risk)):
            worst = max(worst, float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max()))
    print(f"rescoring and MBR of the long lists: max err {worst:.3e}")
    assert worst <= TOL
