"""The identities that tie the eight CTC decoder entry points together, in one place and at the
smallest shapes where a path can still go wrong: G = 2 heads, B = 3 clips of T = 6 frames with
lengths (6, 3, 0), beam 2, and C = 5, C = 2 (K = min(W + 1, C - 1) = 1 label per frame) and
C = 70 (a row spans more than one lane stride).  For greedy, beam, n-best and fused (weight 0,
bonus 0, with a table):

* row g of the grouped call is bitwise the single-head call on head g;
* with collapse_repeats=False, entry 0 of the n-best list is bitwise the 1-best beam result;
* the fused list at weight 0 is bitwise the unfused list;
* a captured graph of every call, replayed on refilled inputs, is bitwise the eager calls.

Everything is compared as bits; the restatements of the searches are in the other decoder files."""
import numpy as np
import pytest
import torch

from tests import nbest_ref as R

pytestmark = pytest.mark.gpu

G, B, T, W = 2, 3, 6, 2
IN_LEN = (6, 3, 0)
CLASSES = (5, 2, 70)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _logits(C, seed):
    return [torch.from_numpy(np.random.default_rng(seed + g).normal(0.0, 4.0, (B, T, C)).astype(np.float32))
            for g in range(G)]


def _calls(S, xs, il, lm):
    """{(mode, collapse, head): outputs}: head None is the grouped call over `xs`, head g the
    single-head call on xs[g]."""
    out = {}
    for g, x in [(None, xs)] + list(enumerate(xs)):
        one = g is not None
        out["greedy", True, g] = S.ctc_greedy_decode_device(x, il) if one else S.ctc_decode_heads_device(x, il, 0)
        for c in (False, True):
            out["beam", c, g] = (S.ctc_decode_device if one else S.ctc_decode_heads_device)(x, il, W, c)
            out["nbest", c, g] = tuple((S.ctc_decode_nbest_device if one else S.ctc_decode_nbest_heads_device)(
                x, il, W, W, c))
            out["fused", c, g] = tuple((S.ctc_decode_fused_nbest_device if one else
                                        S.ctc_decode_fused_nbest_heads_device)(x, il, W, lm, 0.0, 0.0, W, c))
    return out


def _same(a, b, where):
    assert len(a) == len(b), where
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and torch.equal(_bits(u), _bits(v)), (where, i)


def _assert_identities(out):
    for (mode, c, g), res in out.items():
        lead = (G, B) if g is None else (B,)
        listed = mode in ("nbest", "fused")
        assert len(res) == (4 if listed else 3), (mode, c, g)
        assert res[0].shape == lead + ((W, T) if listed else (T,)) and res[-1].shape == lead, (mode, c, g)
        if g is not None:  # row g of the grouped call
            _same([t[g] for t in out[mode, c, None]], res, ("grouped", mode, c, g))
        if mode == "fused":
            _same(res, out["nbest", c, g], ("fused", c, g))
        if mode == "nbest" and not c:  # entry 0 of the uncollapsed list
            _same([t.select(len(lead), 0) for t in res[:3]], out["beam", c, g], ("entry 0", g))
    for b, n in enumerate(IN_LEN):  # the empty clip: the empty hypothesis, a list of one
        if n == 0:
            assert int(out["nbest", True, None][3][:, b].max()) == 1 and not out["beam", True, None][1][:, b].any()
            assert not out["greedy", True, None][1][:, b].any()


@pytest.mark.parametrize("C", CLASSES)
def test_the_decoder_paths_agree_bitwise_eager_and_replayed(C):
    import scattennet_amd as S
    dev = _dev()
    xs = [x.to(dev) for x in _logits(C, 60)]
    il = torch.tensor(IN_LEN, dtype=torch.int32, device=dev)
    lm = S.BigramLM(R.random_lm(C), device=dev)
    _assert_identities(_calls(S, xs, il, lm))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _calls(S, xs, il, lm)  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = _calls(S, xs, il, lm)
    for seed in (None, 80):  # the captured inputs, then refilled ones
        if seed is not None:
            for x, new in zip(xs, _logits(C, seed)):
                x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        eager = _calls(S, xs, il, lm)
        for key, res in captured.items():
            _same(res, eager[key], ("replay", seed) + key)
        _assert_identities(captured)
