"""CTC decoding (greedy, prefix beam search) and WER counts on the device
(scattennet_amd/csrc/decode.hip, scattennet_amd/decode.py) against the float64 restatements
of tests/decode_ref.py, the exhaustive enumeration and the reference's own WER counts
(tests/golden/wer_cases.npz, written by tests/golden/gen_golden_wer.py).

Exact equality of a discrete search only means something away from ties, so every beam case
asserts on the CPU side that its inputs keep the restatement's smallest gap between the last
kept and the first dropped candidate, and between the two best final beams, at or above
MIN_GAP log units.  That is a condition on the inputs (the seeds below were chosen for it),
not a tolerance."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests.golden_util import GOLDEN, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sca_ctc_decode_workspace_bytes", "sca_ctc_greedy_decode", "sca_ctc_beam_decode", "sca_wer_counts")
MIN_GAP = 1e-4
TOL = 1e-3  # the project's relative bound (golden_util.rel_err)
ERR_ARG = 1

# (B, T, C, W) -> (seed, in_len)
BEAM_CASES = {
    (8, 64, 1124, 5): (16, [64, 0, 1, 37, 64, 50, 13, 64]),  # the evaluation shape; ragged with 0, 1 and T
    (3, 37, 70, 1): (0, [37, 20, 5]),                       # odd sizes; beam 1 is not greedy
    (2, 20, 33, 32): (8, [20, 13]),                         # the widest beam
    # fewer labels than W + 1; pruned prefixes come back here while a child of theirs is still active
    (5, 16, 4, 8): (0, [16, 0, 1, 9, 16]),
    (1, 4, 8192, 32): (0, [4]),                             # the class limit
    (2, 128, 12, 8): (0, [128, 97]),                        # outputs of more than 64 tokens (nbest_ref's logits)
}
EXHAUSTIVE_CASE = ((4, 4, 3, 32), 0)


def _logits(shape, seed, std=4.0):
    B, T, C, _ = shape
    return np.random.default_rng(seed).normal(0.0, std, (B, T, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _beam_ref(shape, seed, lens, collapse):
    """The restatement for one random case, computed once and shared."""
    x = _logits(shape, seed)
    return R.beam_search_batch(x, lens, shape[3], collapse)


def _planted():
    """Logits built from frame paths with blanks and repeats, scaled so that the path
    dominates, plus noise.  A = 1, B = 2, C = 3; T = 12, 7 classes."""
    paths = [[1, 1, 0, 1, 2, 2, 0, 0, 3],     # A A _ A B B _ _ C
             [1, 0, 1, 0, 0, 1, 1, 0],        # a run of one label across blanks
             [2, 3, 3, 0]]                    # the final frame is blank
    T, C = 12, 7
    x = np.random.default_rng(0).normal(0.0, 1.0, (len(paths), T, C)).astype(np.float32)
    for b, p in enumerate(paths):
        for t, c in enumerate(p):
            x[b, t, c] += 12.0
    lens = [len(p) for p in paths]
    raw = [[1, 1, 2, 3], [1, 1, 1], [2, 3]]   # the search result: repeats across a blank stay
    merged = [[1, 2, 3], [1], [2, 3]]         # after the reference's groupby
    return x, lens, raw, merged


def _rows(tokens, lengths):
    tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
    return [tokens[b, :lengths[b]].tolist() for b in range(len(lengths))]


def _assert_padded(tokens, lengths):
    tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
    for b in range(len(lengths)):
        assert not tokens[b, lengths[b]:].any(), b


# ------------------------------------------------------------------------------- CPU tests
def test_header_library_and_binding_have_the_entry_points():
    from scattennet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^\s*\w+\s+%s\s*\(" % name, src, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name


def test_argument_validation_makes_no_gpu_call():
    """Unsupported sizes are SCA_ERR_ARG before any launch (NULL pointers: nothing could run)."""
    from scattennet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        argt, rest = _lib.EXPORTS[name]
        getattr(lib, name).argtypes, getattr(lib, name).restype = argt, rest
    beam = lambda B, T, C, W: lib.sca_ctc_beam_decode(None, None, B, T, C, W, 1, None, None, None, None, None)  # noqa: E731
    assert beam(2, 8, 16, 0) == ERR_ARG
    assert beam(2, 8, 16, 33) == ERR_ARG
    assert beam(2, 8, 8193, 5) == ERR_ARG
    assert beam(2, 8, 16, 5) == ERR_ARG  # NULL buffers
    assert lib.sca_ctc_greedy_decode(None, None, 2, 8, 8193, None, None, None, None, None) == ERR_ARG
    assert lib.sca_wer_counts(None, None, None, None, 4, 129, 16, None, None) == ERR_ARG
    assert lib.sca_wer_counts(None, None, None, None, 4, 16, 129, None, None) == ERR_ARG
    size = lib.sca_ctc_decode_workspace_bytes
    assert size(8, 64, 1124, 5) > 0 and size(1, 1, 1, 1) > 0
    assert size(8, 64, 1124, 33) == 0 and size(8, 64, 8193, 5) == 0
    by_t = [size(8, T, 1124, 5) for T in (1, 2, 16, 64, 65, 400)]
    by_w = [size(8, 64, 1124, W) for W in range(1, 33)]
    assert all(a < b for a, b in zip(by_t, by_t[1:])) and all(a < b for a, b in zip(by_w, by_w[1:]))


# The eight decoders: name -> (grouped, mode, the text sca_last_error() holds after a rejection).
_ONE, _HEADS = "B, T >= 1, 1 <= C <= 8192", "1 <= G <= 8 non-null tensors, B, T >= 1, 1 <= C <= 8192"
DECODERS = {
    "sca_ctc_greedy_decode": (False, "greedy", f"sca_ctc_greedy_decode: bad arguments ({_ONE})"),
    "sca_ctc_beam_decode": (False, "beam", f"sca_ctc_beam_decode: bad arguments ({_ONE}, 1 <= beam_width <= 32)"),
    "sca_ctc_greedy_decode_heads": (True, "greedy", f"sca_ctc_greedy_decode_heads: bad arguments ({_HEADS})"),
    "sca_ctc_beam_decode_heads": (True, "beam",
                                  f"sca_ctc_beam_decode_heads: bad arguments ({_HEADS}, 1 <= beam_width <= 32)"),
    "sca_ctc_beam_decode_nbest": (False, "nbest", f"sca_ctc_beam_decode_nbest: bad arguments ({_ONE}, "
                                                  "1 <= nbest <= beam_width <= 32)"),
    "sca_ctc_beam_decode_heads_nbest": (True, "nbest", f"sca_ctc_beam_decode_heads_nbest: bad arguments ({_HEADS}, "
                                                       "1 <= nbest <= beam_width <= 32)"),
    "sca_ctc_beam_decode_fused_nbest": (False, "fused", f"sca_ctc_beam_decode_fused_nbest: bad arguments ({_ONE}, "
                                                        "1 <= nbest <= beam_width <= 32, finite weights)"),
    "sca_ctc_beam_decode_heads_fused_nbest": (True, "fused",
                                              f"sca_ctc_beam_decode_heads_fused_nbest: bad arguments ({_HEADS}, "
                                              "1 <= nbest <= beam_width <= 32, finite weights)"),
}


def _bad_decoder_calls(grouped, mode):
    """The overrides of one valid call (G = 2, B = 2, T = 8, C = 16, W = 5, nbest = 3) that each
    make it unsupported."""
    bad = [{"B": 0}, {"T": 0}, {"C": 0}, {"C": 8193}]
    bad += [{k: None} for k in ("in_len", "tokens", "out_len", "score", "ws", "heads" if grouped else "logits")]
    if mode != "greedy":
        bad += [{"W": 0, "N": 0}, {"W": 33}]
    if mode in ("nbest", "fused"):
        bad += [{"N": 0}, {"N": 6}, {"count": None}]
    if mode == "fused":
        bad += [{"lw": float("inf")}, {"lw": float("nan")}, {"lb": float("-inf")}, {"lb": float("nan")}]
    if grouped:
        bad += [{"G": 0}, {"G": 9}, {"hole": 0}, {"hole": 1}]
    return bad


@pytest.mark.parametrize("name", sorted(DECODERS))
def test_every_decoder_rejects_the_same_bad_arguments_before_any_gpu_call(name):
    """One matrix of unsupported arguments over the eight decoder entry points: each case is
    SCA_ERR_ARG (nothing valid is ever passed, so a launch would crash) and leaves exactly the
    entry point's own message in sca_last_error()."""
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    for sym in (name, "sca_wer_counts", "sca_last_error"):
        getattr(lib, sym).argtypes, getattr(lib, sym).restype = L.EXPORTS[sym]
    grouped, mode, message = DECODERS[name]
    p = ctypes.c_void_p(0x1000)  # never dereferenced
    for over in _bad_decoder_calls(grouped, mode):
        a = dict(G=2, B=2, T=8, C=16, W=5, N=3, lw=0.5, lb=0.25, hole=None, heads=L.DecodeHeads(), logits=p, in_len=p,
                 tokens=p, out_len=p, score=p, count=p, ws=p)
        a.update(over)
        if a["heads"] is not None:
            for g in range(min(max(a["G"], 0), 8)):
                a["heads"].logits[g] = None if g == a["hole"] else 0x1000
        args = [None if a["heads"] is None else ctypes.byref(a["heads"]), a["G"]] if grouped else [a["logits"]]
        args += [a["in_len"], a["B"], a["T"], a["C"]]
        args += {"greedy": [], "beam": [a["W"], 1], "nbest": [a["W"], a["N"], 1],
                 "fused": [a["W"], a["N"], 1, p, a["lw"], a["lb"]]}[mode]
        args += [a["tokens"], a["out_len"], a["score"]] + ([a["count"]] if mode in ("nbest", "fused") else [])
        assert lib.sca_wer_counts(None, None, None, None, 0, 0, 0, None, None) == ERR_ARG  # another message
        assert lib.sca_last_error().decode() != message
        assert getattr(lib, name)(*args, a["ws"], None) == ERR_ARG, over
        assert lib.sca_last_error().decode() == message, over


def test_the_three_workspace_size_functions_are_one_formula():
    from scattennet_amd import _lib as L
    lib = ctypes.CDLL(L.LIB_PATH)
    one, heads, fused = (getattr(lib, n) for n in ("sca_ctc_decode_workspace_bytes",
                                                   "sca_ctc_decode_heads_workspace_bytes",
                                                   "sca_ctc_fused_workspace_bytes"))
    for fn, n in ((one, 4), (heads, 5), (fused, 5)):
        fn.argtypes, fn.restype = [ctypes.c_int] * n, ctypes.c_long
    for B, T, C, W in [(1, 1, 1, 1), (2, 8, 16, 5), (8, 64, 1124, 5), (3, 37, 8192, 32), (5, 400, 2, 1)]:
        want = 4 * (2 * B * T + 2 * B * T * (W + 1)) + 8 * B * (T * W + 1)  # rowstat, cls, clp; the arena
        assert one(B, T, C, W) == heads(1, B, T, C, W) == fused(1, B, T, C, W) == want
        for G in (2, 8):  # the single-head layout over G B clips
            assert heads(G, B, T, C, W) == fused(G, B, T, C, W) == one(G * B, T, C, W)
    for B, T, C, W in [(0, 8, 16, 5), (2, 0, 16, 5), (2, 8, 0, 5), (2, 8, 8193, 5), (2, 8, 16, 0), (2, 8, 16, 33),
                       (-1, 8, 16, 5)]:
        assert one(B, T, C, W) == 0
        for G in (1, 2):
            assert heads(G, B, T, C, W) == 0 and fused(G, B, T, C, W) == 0
    for G in (0, 9, -1):
        assert heads(G, 2, 8, 16, 5) == 0 and fused(G, 2, 8, 16, 5) == 0


@pytest.mark.parametrize("T,C", [(4, 3), (2, 6)])
def test_restatement_matches_exhaustive_enumeration(T, C):
    """All prefixes fit a beam of 32, so the search is exact: it must return the arg-max
    labelling over all C^T paths and its log-probability."""
    for seed in range(10):
        x = np.random.default_rng(100 + seed).normal(0.0, 2.0, (T, C))
        acc = R.exhaustive(x)
        best = max(acc, key=acc.get)
        labels, score, _, _ = R.beam_search(x, T, 32)
        assert tuple(labels) == best, seed
        assert abs(score - acc[best]) < 1e-9, seed


@pytest.mark.parametrize("T,C,W", [(64, 1124, 5), (37, 70, 1), (20, 33, 32), (16, 4, 8)])
def test_restatement_preselection_is_exact(T, C, W):
    """Candidates from the W + 1 best labels of a frame only: same labelling, same score."""
    x = np.random.default_rng(3).normal(0.0, 4.0, (T, C))
    full = R.beam_search(x, T, W)
    pre = R.beam_search(x, T, W, preselect=True)
    assert full[0] == pre[0] and abs(full[1] - pre[1]) < 1e-9


def _wer_fixture():
    with np.load(os.path.join(GOLDEN, "wer_cases.npz")) as z:
        return {k: z[k] for k in z.files}


def test_wer_restatement_and_rates_match_reference_fixture():
    from scattennet_amd import decode
    z = _wer_fixture()
    N = len(z["counts"])
    refs = [z["ref"][n, :z["ref_len"][n]].tolist() for n in range(N)]
    hyps = [z["hyp"][n, :z["hyp_len"][n]].tolist() for n in range(N)]
    for n in range(N):
        assert R.wer_single(refs[n], hyps[n]) == tuple(z["counts"][n]), z["tags"][n]
    subsets = [k[len("subset_"):-len("_idx")] for k in z if k.endswith("_idx")]
    assert len(subsets) == 4
    for name in subsets:
        idx = z[f"subset_{name}_idx"]
        want = dict(zip(("wer", "del_rate", "ins_rate", "sub_rate"), z[f"subset_{name}_rates"]))
        got = decode.wer_from_counts(torch.from_numpy(z["counts"][idx]))
        restated = R.wer_list([refs[i] for i in idx], [hyps[i] for i in idx])
        for k, v in want.items():
            assert got[k] == pytest.approx(v, rel=1e-12), (name, k)
            assert restated[k] == pytest.approx(v, rel=1e-12), (name, k)


def test_cpu_logits_and_bad_host_lengths_are_refused():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_decode_device(x, torch.tensor([8, 8]), beam_size=5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_greedy_decode_device(x, torch.tensor([8, 8]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.wer_counts(torch.zeros(2, 4, dtype=torch.int32), torch.tensor([1, 1]),
                     torch.zeros(2, 4, dtype=torch.int32), torch.tensor([1, 1]))
    # host lengths are validated before anything touches the device
    with pytest.raises(RuntimeError, match="one per clip"):
        S.ctc_decode_device(x, torch.tensor([8, 8, 8]), beam_size=5)
    with pytest.raises(RuntimeError, match="at most 8"):
        S.ctc_decode(x, 5, torch.tensor([8, 9]))
    with pytest.raises(RuntimeError, match="non-negative"):
        S.ctc_greedy_decode_device(x, torch.tensor([8, -1]))
    with pytest.raises(ValueError, match="beam_size"):
        S.ctc_decode_device(x, torch.tensor([8, 8]), beam_size=33)


# ------------------------------------------------------------------------------- GPU tests
@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(BEAM_CASES), ids=lambda s: "B%d_T%d_C%d_W%d" % s)
@pytest.mark.parametrize("collapse", [False, True])
def test_hip_beam_decode_matches_restatement(shape, collapse):
    import scattennet_amd as S
    seed, lens = BEAM_CASES[shape]
    want, want_score, frame_gap, final_gap = _beam_ref(shape, seed, tuple(lens), collapse)
    print("gaps", shape, frame_gap, final_gap)
    assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP  # a condition on the inputs
    x = torch.from_numpy(_logits(shape, seed)).cuda()
    tokens, lengths, scores = S.ctc_decode_device(x, torch.tensor(lens), beam_size=shape[3], collapse_repeats=collapse)
    assert tokens.shape == (shape[0], shape[1]) and tokens.dtype == torch.int32 and lengths.dtype == torch.int32
    assert _rows(tokens, lengths) == want
    _assert_padded(tokens, lengths)
    err = rel_err(scores, torch.from_numpy(want_score))
    print("score rel err", shape, err)
    assert err < TOL
    for b, n in enumerate(lens):
        if n == 0:
            assert lengths[b].item() == 0 and scores[b].item() == 0.0


@pytest.mark.gpu
def test_hip_beam_decode_matches_exhaustive_enumeration():
    import scattennet_amd as S
    shape, seed = EXHAUSTIVE_CASE
    B, T, C, W = shape
    x = _logits(shape, seed, std=2.0)
    _, _, _, final_gap = R.beam_search_batch(x, [T] * B, W)
    assert final_gap >= MIN_GAP
    tokens, lengths, scores = S.ctc_decode_device(torch.from_numpy(x).cuda(), torch.tensor([T] * B), beam_size=W,
                                                  collapse_repeats=False)
    got = _rows(tokens, lengths)
    want = []
    for b in range(B):
        acc = R.exhaustive(x[b])
        best = max(acc, key=acc.get)
        assert tuple(got[b]) == best, b
        want.append(acc[best])
    assert rel_err(scores, torch.tensor(want)) < TOL


@pytest.mark.gpu
def test_hip_beam_decode_planted_paths():
    import scattennet_amd as S
    x, lens, raw, merged = _planted()
    for collapse, expect in ((False, raw), (True, merged)):
        want, want_score, frame_gap, final_gap = R.beam_search_batch(x, lens, 4, collapse)
        assert want == expect  # the restatement itself: repeats across a blank, parent merge
        assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP
        tokens, lengths, scores = S.ctc_decode_device(torch.from_numpy(x).cuda(), torch.tensor(lens), beam_size=4,
                                                      collapse_repeats=collapse)
        assert _rows(tokens, lengths) == expect
        assert all(n < t for n, t in zip(lengths.tolist(), lens))  # shorter than the clips
        _assert_padded(tokens, lengths)
        assert rel_err(scores, torch.from_numpy(want_score)) < TOL
    assert raw != merged


def _torch_greedy(x, lens):
    out = []
    for b, n in enumerate(lens):
        path = torch.unique_consecutive(x[b, :n].argmax(-1))
        out.append(path[path != 0].tolist())
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,T,C,lens", [(8, 64, 1124, [64, 0, 1, 37, 64, 50, 13, 64]), (3, 37, 70, [37, 20, 1]),
                                        (2, 128, 12, [128, 97])])
def test_hip_greedy_decode_matches_torch(B, T, C, lens):
    import scattennet_amd as S
    # a small spread, so that blanks and repeats do occur among the arg-maxima
    xn = np.random.default_rng(11).normal(0.0, 1.0, (B, T, C)).astype(np.float32)
    xn[:, :, 0] += 3.0 * (np.random.default_rng(12).random((B, T)) < 0.3)
    for t in range(1, T, 3):
        xn[:, t] = xn[:, t - 1]  # repeated frames
    x = torch.from_numpy(xn).cuda()
    tokens, lengths, scores = S.ctc_greedy_decode_device(x, torch.tensor(lens))
    want = _torch_greedy(x.cpu(), lens)
    assert _rows(tokens, lengths) == want
    assert any(len(w) < n for w, n in zip(want, lens) if n > 1)
    _assert_padded(tokens, lengths)
    ref = np.array([R.greedy(xn[b], lens[b])[1] for b in range(B)])
    assert [R.greedy(xn[b], lens[b])[0] for b in range(B)] == want
    assert rel_err(scores, torch.from_numpy(ref)) < TOL


@pytest.mark.gpu
def test_hip_greedy_tie_goes_to_the_lower_class():
    import scattennet_amd as S
    x = torch.full((1, 3, 70), -1.0)
    x[0, 0, 5] = x[0, 0, 3] = x[0, 0, 69] = 2.0   # 3, 5 and 69 tie -> 3
    x[0, 1, 0] = x[0, 1, 2] = 2.0                 # blank and 2 tie -> blank
    x[0, 2, 66] = x[0, 2, 4] = 2.0                # two waves' lanes tie -> 4
    tokens, lengths, _ = S.ctc_greedy_decode_device(x.cuda(), torch.tensor([3]))
    assert _rows(tokens, lengths) == [[3, 4]]


@pytest.mark.gpu
def test_hip_decode_under_graph_capture():
    import scattennet_amd as S
    shape = (8, 64, 1124, 5)
    seed, lens = BEAM_CASES[shape]
    xs = [torch.from_numpy(_logits(shape, s)).cuda() for s in (seed, seed + 1)]
    il = torch.tensor(lens, dtype=torch.int32).cuda()
    eager = [S.ctc_decode_device(x, il, beam_size=5) for x in xs]
    static = xs[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.ctc_decode_device(static, il, beam_size=5)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = S.ctc_decode_device(static, il, beam_size=5)
    for k in (0, 1, 0):
        static.copy_(xs[k])
        g.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager[k]):
            assert torch.equal(got, want), k
    assert not torch.equal(eager[0][0], eager[1][0])


@pytest.mark.gpu
def test_hip_ctc_decode_list_form_and_decode_outputs():
    import scattennet_amd as S
    x, lens, _, merged = _planted()
    got = S.ctc_decode(torch.from_numpy(x).cuda(), 4, torch.tensor(lens))
    assert got == merged and all(isinstance(t, int) for row in got for t in row)
    torch.manual_seed(0)
    B, T, C = 2, 8, 12
    cfg = {"residual_blocks": [64], "out_fusion_dim": 64, "alignment_module": {"input_size": 64, "hidden_size": 64}}
    head = S.RecognitionHead(cfg, C).cuda().eval()
    feats = [torch.randn(B, T, 64, device="cuda") * 4 for _ in range(4)]
    with torch.no_grad():
        out = head(feats[0], feats[1], feats[2], feats[3])
    out["input_lengths"] = torch.tensor([8, 5])
    out["total_loss"] = torch.zeros((), device="cuda")
    dec = S.decode_outputs(out, beam_size=5)
    assert sorted(dec) == ["alignment_", "fuse_coord_"]
    for name, rows in dec.items():
        z = out[name + "gloss_logits"].cpu().numpy()
        want, _, frame_gap, final_gap = R.beam_search_batch(z, [8, 5], 5, True)
        assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP
        assert rows == want, name


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_hip_decode_reduced_precision_logits_take_the_fp32_path(dtype):
    import scattennet_amd as S
    x, lens, _, merged = _planted()
    xh = torch.from_numpy(x).cuda().to(dtype)
    got = S.ctc_decode_device(xh, torch.tensor(lens), beam_size=4)
    want = S.ctc_decode_device(xh.float(), torch.tensor(lens), beam_size=4)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].dtype == dtype and torch.equal(got[2], want[2].to(dtype))
    assert _rows(got[0], got[1]) == merged  # the planted paths dominate by far more than the rounding


@pytest.mark.gpu
def test_hip_wer_counts_fixture_and_random_pairs():
    import scattennet_amd as S
    z = _wer_fixture()
    got = S.wer_counts(torch.from_numpy(z["ref"]).cuda(), torch.from_numpy(z["ref_len"]),
                       torch.from_numpy(z["hyp"]).cuda(), torch.from_numpy(z["hyp_len"]))
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == z["counts"].tolist()
    rng = np.random.default_rng(5)
    N = 64
    rl = rng.integers(0, 129, N)
    hl = rng.integers(0, 129, N)
    rl[:4], hl[:4] = [128, 0, 128, 1], [128, 128, 0, 127]
    ref = np.zeros((N, 128), np.int32)
    hyp = np.zeros((N, 128), np.int32)
    for n in range(N):
        vocab = 2 + n % 7  # few distinct tokens: many equal cells and ties in the back-trace
        ref[n, :rl[n]] = rng.integers(1, vocab + 1, rl[n])
        if n % 2:  # a hypothesis derived from the reference
            keep = ref[n, :rl[n]][rng.random(rl[n]) > 0.15][:hl[n]]
            hl[n] = len(keep)
            hyp[n, :hl[n]] = np.where(rng.random(hl[n]) < 0.15, rng.integers(1, vocab + 1, hl[n]), keep)
        else:
            hyp[n, :hl[n]] = rng.integers(1, vocab + 1, hl[n])
    want = [list(R.wer_single(ref[n, :rl[n]], hyp[n, :hl[n]])) for n in range(N)]
    got = S.wer_counts(torch.from_numpy(ref).cuda(), torch.from_numpy(rl.astype(np.int32)).cuda(),
                       torch.from_numpy(hyp).cuda(), torch.from_numpy(hl.astype(np.int32)).cuda())
    assert got.cpu().numpy().tolist() == want


@pytest.mark.gpu
def test_hip_decode_chained_into_wer_counts_on_the_device():
    import scattennet_amd as S
    shape = (8, 64, 1124, 5)
    seed, lens = BEAM_CASES[shape]
    x = torch.from_numpy(_logits(shape, seed)).cuda()
    refs = np.random.default_rng(9).integers(1, 1124, (8, 12)).astype(np.int32)
    ref_len = np.array([12, 3, 0, 7, 12, 9, 1, 5], np.int32)
    tokens, lengths, _ = S.ctc_decode_device(x, torch.tensor(lens, dtype=torch.int32).cuda(), beam_size=5)
    counts = S.wer_counts(torch.from_numpy(refs).cuda(), torch.from_numpy(ref_len).cuda(), tokens, lengths)
    hyps, _, _, _ = _beam_ref(shape, seed, tuple(lens), True)
    want = [list(R.wer_single(refs[b, :ref_len[b]], hyps[b])) for b in range(8)]
    assert counts.cpu().numpy().tolist() == want
    rates = S.wer_from_counts(counts)
    assert rates == R.wer_list([refs[b, :ref_len[b]] for b in range(8)], hyps)
