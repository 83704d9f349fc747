"""CTC forced alignment on the MI355X (scattennet_amd/align.py; csrc/align.hip:
sca_ctc_align_heads, sca_eval_log_alignments) against the float64 restatement of
tests/align_ref.py, against the greedy decoder, bitwise across its own forms, and inside the
evaluation step on the reference's fixture.

A Viterbi path is a discrete choice, so equality with the restatement only means something away
from ties.  Always asserted: the device path collapses to the labels, spans and frame_label
describe one path, the score and the float64 log-probability of the DEVICE's path are within
the project's bound of the restatement's optimum.  frame_label and spans are compared exactly
for every clip whose restatement gap is at least 4 T_b 2^-24 max(1, |score|): the worst-case
rounding of a T_b-term fp32 running sum, doubled for the two sums compared and doubled again for
the roundings of lp; at most 10 % of a case's feasible clips may fall under that margin."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import align_ref as R
from tests.golden_util import load

pytestmark = pytest.mark.gpu

TOL = 1e-3  # the project's relative bound
GARBAGE = 0x7F7F7F7F

# (B, T, C, S)
SHAPES = [
    (16, 24, 5, 6),
    (16, 40, 20, 12),
    (16, 70, 12, 32),     # L crosses one wave at S_b = 31 / 32
    (16, 140, 9, 64),     # L crosses 128
    (16, 64, 1124, 24),   # the evaluation shape; C is no multiple of 64
    (2, 530, 4, 257),     # L crosses 512: the 1024-thread kernel, back-pointers in global memory
    (1, 1030, 3, 1023),   # the S limit
]
IDS = ["B%d_T%d_C%d_S%d" % s for s in SHAPES]
# The exact-comparison margin grows with T_b |score|: a clip of hundreds of frames that is free to
# place its labels has some decision closer than that, so the two long cases leave the path only
# a few frames of slack (its decisions are then between whole shifted alignments, far apart), and
# their seeds were chosen, on the CPU with the restatement alone, for gaps above the margin.
SEEDS = {(2, 530, 4, 257): 100, (1, 1030, 3, 1023): 122}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(shape, seed=0):
    """(x, in_len, labels, lab_len, refs) of one random case: logits 3 N(0, 1), ragged lengths,
    one clip in three with an adjacent repeated label; clip 0 has S labels and clip 1 has S - 1,
    both over all T frames.  refs: the restatement per clip, computed once and shared."""
    B, T, C, S = shape
    rng = np.random.default_rng(SEEDS.get(shape, 100) + seed + 7 * S)
    x = (3.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    labels = np.zeros((B, S), np.int32)
    in_len, lab_len = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        if S == 1023:  # T_b = the needed length + 3: alternating labels with four repeats
            row = np.array([1 + (j % 2) for j in range(S)])
            for at in (100, 400, 700, 1000):
                row[at:] = 3 - row[at:]
            labels[b], lab_len[b] = row, S
            assert R.needed_frames(row) == S + 4
            in_len[b] = R.needed_frames(row) + 3
            continue
        if S == 257:  # L = 515 and 511; a few frames of slack, as above (see SEEDS)
            lab_len[b] = (257, 255)[b]
            labels[b, :lab_len[b]] = rng.integers(1, C, lab_len[b])
            in_len[b] = R.needed_frames(labels[b, :lab_len[b]]) + 3 - b
            continue
        in_len[b] = T if b < 2 else rng.integers(T // 2, T + 1)
        lab_len[b] = (S, S - 1)[b] if b < 2 else rng.integers(0, min(S, in_len[b] // 2) + 1)
        labels[b, :lab_len[b]] = rng.integers(1, C, lab_len[b])
        if b % 3 == 2 and lab_len[b] >= 2:
            at = rng.integers(0, lab_len[b] - 1)
            labels[b, at + 1] = labels[b, at]
    refs = [R.align(x[b], in_len[b], labels[b, :lab_len[b]]) for b in range(B)]
    return x, in_len, labels, lab_len, refs


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    """Two Alignment tuples, bitwise."""
    return (torch.equal(a.frame_label, b.frame_label) and torch.equal(a.spans, b.spans) and
            torch.equal(_bits(a.conf), _bits(b.conf)) and torch.equal(_bits(a.scores), _bits(b.scores)))


def _check_against_restatement(x, in_len, labels, lab_len, refs, res, min_exact=0.9, label=""):
    """The module docstring's assertions for one head's result (device tensors of B clips)."""
    B, T, _ = x.shape
    S = labels.shape[1]
    fl, spans = res.frame_label.cpu().numpy(), res.spans.cpu().numpy()
    conf, scores = res.conf.float().cpu().numpy(), res.scores.float().cpu().numpy()
    assert fl.shape == (B, T) and spans.shape == (B, S, 2) and conf.shape == (B, S) and scores.shape == (B,)
    feasible = exact = 0
    for b in range(B):
        T_b, S_b = min(max(int(in_len[b]), 0), T), min(max(int(lab_len[b]), 0), S)
        lab = labels[b, :S_b].tolist()
        score, path, r_fl, r_spans, r_conf, gap = refs[b]
        assert (fl[b, T_b:] == -1).all() and not spans[b, S_b:].any() and not conf[b, S_b:].any(), (label, b)
        if path is None:
            assert scores[b] == -np.inf and (fl[b] == -1).all() and not spans[b].any() and not conf[b].any(), (label, b)
            continue
        feasible += 1
        # the device's own path: it collapses to the labels, and the spans describe it
        assert ((fl[b, :T_b] >= -1) & (fl[b, :T_b] < max(S_b, 1))).all(), (label, b)
        dpath = [0 if j < 0 else lab[j] for j in fl[b, :T_b]]
        idx = [j for t, j in enumerate(fl[b, :T_b]) if j >= 0 and (t == 0 or fl[b, t - 1] != j)]
        assert idx == list(range(S_b)) and R.collapse(dpath) == lab, (label, b)
        lp = R.log_softmax(x[b, :T_b]) if T_b else None
        for j in range(S_b):
            s, e = spans[b, j]
            assert 0 <= s < e <= T_b and (fl[b, s:e] == j).all() and (fl[b, :T_b] == j).sum() == e - s, (label, b, j)
            assert abs(conf[b, j] - np.exp(lp[s:e, lab[j]]).mean()) <= 1e-3, (label, b, j)
        bound = TOL * max(1.0, abs(score))
        assert abs(scores[b] - score) <= bound, (label, b, scores[b], score)
        assert abs(R.path_logprob(x[b], dpath) - score) <= bound, (label, b)
        if gap >= 4 * T_b * 2.0 ** -24 * max(1.0, abs(score)):
            exact += 1
            assert fl[b].tolist() == r_fl.tolist() and spans[b, :S_b].tolist() == r_spans.tolist(), (label, b, gap)
            assert np.abs(conf[b, :S_b] - r_conf).max(initial=0.0) <= 1e-3, (label, b)
    print(f"{label}: {feasible} feasible clips, {exact} compared exactly")
    assert feasible > 0 and exact >= min_exact * feasible, (label, feasible, exact)
    return feasible


# ------------------------------------------------------------------ 1: random cases
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_align_random_cases_against_the_restatement(shape):
    import scattennet_amd as S
    dev = _dev()
    x, in_len, labels, lab_len, refs = _case(shape)
    res = S.ctc_align_device(torch.from_numpy(x).to(dev), torch.from_numpy(in_len), torch.from_numpy(labels),
                             torch.from_numpy(lab_len))
    assert res.frame_label.dtype == torch.int32 and res.spans.dtype == torch.int32
    assert res.conf.dtype == torch.float32 and res.scores.dtype == torch.float32
    feasible = _check_against_restatement(x, in_len, labels, lab_len, refs, res, label=IDS[SHAPES.index(shape)])
    assert feasible >= min(shape[0], 8)  # the cases do exercise the recursion


# ------------------------------------------------------------------ 2: edge cases
def _raw_align(xs, in_len, labels, lab_len, per_head):
    """sca_ctc_align_heads through the C ABI on outputs pre-filled with garbage."""
    from scattennet_amd import _lib as L
    G, (B, T, C), S = len(xs), xs[0].shape, labels.shape[-1]
    dev = xs[0].device
    lib = L.lib()
    fl = torch.full((G, B, T), GARBAGE, dtype=torch.int32, device=dev)
    spans = torch.full((G, B, S, 2), GARBAGE, dtype=torch.int32, device=dev)
    conf = torch.full((G, B, S), float("nan"), device=dev)
    scores = torch.full((G, B), float("nan"), device=dev)
    nbytes = lib.sca_ctc_align_workspace_bytes(G, B, T, S)
    assert nbytes > 0
    ws = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=dev)
    hx = L.DecodeHeads()
    for g, x in enumerate(xs):
        hx.logits[g] = x.data_ptr()
    L.check(lib.sca_ctc_align_heads(ctypes.byref(hx), G, L.ptr(in_len), L.ptr(labels), L.ptr(lab_len), per_head, B, T,
                                    C, S, L.ptr(fl), L.ptr(spans), L.ptr(conf), L.ptr(scores), L.ptr(ws),
                                    L.stream_handle()), "sca_ctc_align_heads")
    import scattennet_amd as S_
    return S_.align.Alignment(fl, spans, conf, scores)


def test_align_edge_cases_in_one_batch():
    dev = _dev()
    T, C, S = 12, 6, 5
    rng = np.random.default_rng(5)
    #          all blank   nothing   no frames  forced        one short     in_len > T       lab_len > S
    in_len = [12,          0,        0,         4,            3,            99,              10]
    lab_len = [0,          0,        3,         3,            3,            5,               99]
    rows = [[],            [],       [1, 2, 3], [2, 2, 3],    [2, 2, 3],    [1, 5, 5, 2, 4], [3, 1, 4, 1, 5]]
    B = len(rows)
    labels = np.zeros((B, S), np.int32)
    for b, r in enumerate(rows):
        labels[b, :len(r)] = r
    labels[0] = 4  # padding beyond lab_len is never read as a label
    x = (3.0 * rng.standard_normal((B, T, C))).astype(np.float32)
    t = lambda a: torch.as_tensor(np.asarray(a, np.int32)).to(dev)  # noqa: E731  device lengths: trusted
    res = _raw_align([torch.from_numpy(x).to(dev)], t(in_len), t(labels), t(lab_len), 0)
    res = type(res)(*(v[0] for v in res))
    refs = [R.align(x[b], in_len[b], rows[b]) for b in range(B)]
    _check_against_restatement(x, in_len, labels, lab_len, refs, res, min_exact=1.0, label="edge")
    fl, spans = res.frame_label.cpu().numpy(), res.spans.cpu().numpy()
    conf, scores = res.conf.cpu().numpy(), res.scores.cpu().numpy()
    # nothing of the garbage is left
    assert not (fl == GARBAGE).any() and not (spans == GARBAGE).any()
    assert not np.isnan(conf).any() and not np.isnan(scores).any()
    lp = [R.log_softmax(x[b]) for b in range(B)]
    assert (fl[0] == -1).all() and abs(scores[0] - lp[0][:, 0].sum()) <= TOL * abs(lp[0][:, 0].sum())
    assert scores[1] == 0.0 and (fl[1] == -1).all()
    assert scores[2] == -np.inf and scores[4] == -np.inf
    assert fl[3].tolist() == [0, -1, 1, 2] + [-1] * 8 and spans[3, :3].tolist() == [[0, 1], [2, 3], [3, 4]]
    assert abs(scores[3] - (lp[3][0, 2] + lp[3][1, 0] + lp[3][2, 2] + lp[3][3, 3])) <= TOL * abs(scores[3])
    assert refs[5][1] is not None and len(refs[5][1]) == T and (fl[5] >= 0).sum() >= 5  # clamped to T
    assert refs[6][1] is not None and (spans[6, :, 1] > spans[6, :, 0]).all()  # clamped to S


# ------------------------------------------------------------------ 3: exact ties
@pytest.mark.parametrize("T,rows", [(9, [[1, 2, 3]]), (70, [list(1 + np.arange(33) % 4)]),
                                    (12, [[1, 1, 2, 2, 1], [3, 3, 3]])], ids=["T9_S3", "T70_S33", "repeats"])
def test_align_exact_ties_follow_the_tie_rules(T, rows):
    """All-equal logits: every path ties and every reachable state of a frame holds the same
    fp32 value, so the device result is the restatement's exactly."""
    import scattennet_amd as S
    dev = _dev()
    B, C, Smax = len(rows), 5, max(len(r) for r in rows)
    labels = np.zeros((B, Smax), np.int32)
    for b, r in enumerate(rows):
        labels[b, :len(r)] = r
    lab_len = np.array([len(r) for r in rows], np.int32)
    x = np.full((B, T, C), 0.75, np.float32)
    res = S.ctc_align_device(torch.from_numpy(x).to(dev), torch.full((B,), T), torch.from_numpy(labels),
                             torch.from_numpy(lab_len))
    for b, r in enumerate(rows):
        score, path, r_fl, r_spans, r_conf, gap = R.align(x[b], T, r)
        assert gap == 0.0 and path is not None
        assert res.frame_label[b].cpu().numpy().tolist() == r_fl.tolist()
        assert res.spans[b, :len(r)].cpu().numpy().tolist() == r_spans.tolist()
        assert abs(float(res.scores[b]) - score) <= TOL * abs(score)
        assert np.abs(res.conf[b, :len(r)].cpu().numpy() - r_conf).max() <= 1e-3


# ------------------------------------------------------------------ 4: the greedy decoder
def test_align_of_greedy_hypotheses_reproduces_the_best_path():
    import scattennet_amd as S
    dev = _dev()
    B, T, C = 8, 37, 9
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, T, C)).astype(np.float32) * 2
    x[:, :, 0] += 3.0 * (rng.random((B, T)) < 0.4)  # blanks occur
    for t in range(1, T, 3):
        x[:, t] = x[:, t - 1]  # and repeated frames
    top = np.sort(x, axis=-1)
    assert float((top[..., -1] - top[..., -2]).min()) > 1e-3  # no arg-max near a tie (on the inputs)
    in_len = np.array([37, 30, 1, 19, 37, 0, 25, 8], np.int32)
    xd, il = torch.from_numpy(x).to(dev), torch.from_numpy(in_len).to(dev)
    tokens, lengths, gscores = S.ctc_greedy_decode_device(xd, il)
    res = S.ctc_align_device(xd, il, tokens, lengths)  # the decoder's device tensors as they are
    sc, gs = res.scores.cpu().numpy().astype(np.float64), gscores.cpu().numpy().astype(np.float64)
    assert (np.abs(sc - gs) <= TOL * np.maximum(1.0, np.abs(gs))).all(), (sc, gs)
    spans, n = res.spans.cpu().numpy(), lengths.cpu().numpy()
    for b in range(B):
        am = x[b, :in_len[b]].argmax(-1)
        j = -1
        for t, c in enumerate(am):
            if c != 0 and (t == 0 or am[t - 1] != c):
                j += 1
            if c != 0:
                assert spans[b, j, 0] <= t < spans[b, j, 1], (b, t, j)
        assert j + 1 == n[b]


# ------------------------------------------------------------------ 5: bitwise forms
def _heads_case(G, dev):
    shape = (16, 70, 12, 32)
    _, in_len, labels, lab_len, _ = _case(shape)
    xs = [torch.from_numpy(_case(shape, seed=g)[0]).to(dev) for g in range(G)]
    return xs, torch.from_numpy(in_len), torch.from_numpy(labels), torch.from_numpy(lab_len)


@pytest.mark.parametrize("G", [1, 2, 5])
def test_grouped_align_is_bitwise_the_single_head_call(G):
    import scattennet_amd as S
    dev = _dev()
    xs, il, lab, n = _heads_case(G, dev)
    shared = S.ctc_align_heads_device(xs, il, lab, n)
    assert shared.frame_label.shape == (G, 16, 70) and shared.spans.shape == (G, 16, 32, 2)
    assert shared.conf.shape == (G, 16, 32) and shared.scores.shape == (G, 16)
    for g in range(G):
        one = S.ctc_align_device(xs[g], il, lab, n)
        assert _same(type(one)(*(v[g] for v in shared)), one), g
    # one label set per head: tiled labels give the shared call bitwise ...
    tiled = S.ctc_align_heads_device(xs, il, lab.expand(G, *lab.shape), n.expand(G, -1))
    assert _same(tiled, shared)
    # ... and different sets per head give each head's own single call
    labs = torch.stack([torch.roll(lab, g, 0) for g in range(G)])
    ns = torch.stack([torch.roll(n, g, 0) for g in range(G)])
    own = S.ctc_align_heads_device(xs, il, labs, ns)
    for g in range(G):
        assert _same(type(own)(*(v[g] for v in own)), S.ctc_align_device(xs[g], il, labs[g], ns[g])), g
    if G > 1:
        assert not torch.equal(shared.frame_label[0], shared.frame_label[1])  # the heads do differ


def test_captured_align_replayed_on_refilled_inputs_equals_eager():
    import scattennet_amd as S
    dev = _dev()
    xs, il, lab, n = _heads_case(2, dev)
    il, lab, n = il.to(dev).int(), lab.to(dev), n.to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.ctc_align_heads_device(xs, il, lab, n)  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.ctc_align_heads_device(xs, il, lab, n)
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, S.ctc_align_heads_device(xs, il, lab, n))
    # refill the static inputs: other logits, lengths and labels
    xs[0].copy_(torch.from_numpy(_case((16, 70, 12, 32), seed=3)[0]))
    xs[1].copy_(torch.from_numpy(_case((16, 70, 12, 32), seed=4)[0]))
    il.copy_(torch.roll(il, 3))
    lab.copy_(torch.roll(lab, 5, 0))
    n.copy_(torch.roll(n, 5))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(out, S.ctc_align_heads_device(xs, il, lab, n))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_align_reduced_precision_logits_take_the_fp32_path(dtype):
    import scattennet_amd as S
    dev = _dev()
    xs, il, lab, n = _heads_case(2, dev)
    low = [x.to(dtype) for x in xs]
    got = S.ctc_align_heads_device(low, il, lab, n)
    want = S.ctc_align_heads_device([x.float() for x in low], il, lab, n)
    assert torch.equal(got.frame_label, want.frame_label) and torch.equal(got.spans, want.spans)
    assert got.conf.dtype == dtype and torch.equal(got.conf, want.conf.to(dtype))
    assert got.scores.dtype == dtype and torch.equal(got.scores, want.scores.to(dtype))


# ------------------------------------------------------------------ 6: the evaluation step
def _build(fx, dev):
    import scattennet_amd as S
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


def _src(fx, dev):
    return {k: v.to(dev) for k, v in fx["in"].items()}


def _lists(state, tokens, lengths, res):
    """What EvalState.alignments() must hold for one step, from the step's device results."""
    import scattennet_amd as S
    from scattennet_amd.evaluate import logits_name
    G, B = lengths.shape
    per_head = [S.alignment_lists(tokens[g].cpu().numpy(), lengths[g].cpu().numpy(), res.spans[g].cpu().numpy(),
                                  res.conf[g].cpu().numpy(), res.scores[g].cpu().numpy()) for g in range(G)]
    return [{logits_name(k): per_head[g][b] for g, k in enumerate(state.heads)} for b in range(B)]


def test_eval_step_with_align_changes_nothing_else_and_logs_the_alignments(fx):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = _src(fx, dev)
    plain_state = S.EvalState(model, capacity=9, log_width=13)
    plain = [S.eval_step(model, src, plain_state) for _ in range(3)][0]
    assert "spans" not in plain and "conf" not in plain and "align_scores" not in plain

    state = S.EvalState(model, capacity=9, log_width=13, align=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = S.eval_step(model, src, state)  # step 1: eager
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out["tokens"], plain["tokens"]) and torch.equal(out["lengths"], plain["lengths"])
    assert torch.equal(out["counts"], plain["counts"])
    assert out["spans"].shape == (2, 3, 13, 2) and out["conf"].shape == (2, 3, 13)
    assert out["align_scores"].shape == (2, 3)
    logits = [out[k] for k in state.heads]
    res = S.ctc_align_heads_device(logits, out["input_lengths"], out["tokens"], out["lengths"])
    assert torch.equal(out["spans"], res.spans) and torch.equal(_bits(out["conf"]), _bits(res.conf))
    assert torch.equal(_bits(out["align_scores"]), _bits(res.scores))
    # every hypothesis can be emitted by its own logits, and the spans lie inside the clip
    assert bool(torch.isfinite(res.scores).all())
    il = out["input_lengths"].cpu().numpy()
    sp, n = res.spans.cpu().numpy(), out["lengths"].cpu().numpy()
    for g in range(2):
        for b in range(3):
            assert (sp[g, b, :n[g, b], 1] <= il[b]).all() and (sp[g, b, :n[g, b], 1] > sp[g, b, :n[g, b], 0]).all()
    want_step = _lists(state, out["tokens"], out["lengths"], res)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap = S.eval_step(model, src, state)  # captured: not a step yet
    graph.replay()  # steps 2 and 3
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap["spans"], out["spans"]) and torch.equal(cap["tokens"], out["tokens"])
    raw = state.raw()
    assert raw["cursor"] == 9 and raw["steps"] == 3 and raw["overflow"] == 0
    assert state.read() == plain_state.read()
    assert state.hypotheses() == plain_state.hypotheses()
    got = state.alignments()
    assert len(got) == 9 and got == want_step * 3
    assert sorted(got[0]) == ["alignment_", "fuse_coord_"]
    hyps = state.hypotheses()
    for r in range(9):  # an alignment names its hypothesis's glosses, in order
        for name in got[r]:
            assert [e[0] for e in got[r][name]] == hyps[r][name]
    scaled = state.alignments(frame_scale=2)
    assert [(c, 2 * s, 2 * e, p) for c, s, e, p in got[4]["fuse_coord_"]] == scaled[4]["fuse_coord_"]
    state.reset()
    assert state.alignments() == [] and not state.span_log.any() and not state.conf_log.any()


@pytest.fixture(scope="module")
def eager_alignment(fx):
    """The unpadded eager eval_step with alignment of the fixture batch (T = 26), once."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    state = S.EvalState(model, capacity=3, log_width=13, align=True)
    out = S.eval_step(model, _src(fx, dev), state)
    return {"spans": out["spans"].cpu(), "conf": out["conf"].cpu(), "tokens": out["tokens"].cpu(),
            "alignments": state.alignments()}


@pytest.mark.parametrize("bucket", [28, 32, 40])
def test_bucketed_eval_step_alignment_equals_the_unpadded_eager_step(fx, eager_alignment, bucket):
    """Three feeds: the eager, the capture and the replay path of the bucket."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = _src(fx, dev)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(bucket,), label_bucket=3, capacity=9, align=True)
    want = eager_alignment
    for i in range(3):
        out = bes.step(src)
        assert out["spans"].shape == (2, 3, 13, 2) and out["conf"].shape == (2, 3, 13), (bucket, i)
        assert torch.equal(out["tokens"].cpu(), want["tokens"]), (bucket, i)
        assert torch.equal(out["spans"].cpu(), want["spans"]), (bucket, i)
        assert float((out["conf"].cpu() - want["conf"]).abs().max()) <= 1e-3, (bucket, i)
    assert bes.graphs_captured == 1
    got = bes.alignments()
    assert len(got) == 9
    for r in range(9):
        for name, entries in want["alignments"][r % 3].items():
            assert [e[:3] for e in got[r][name]] == [e[:3] for e in entries], (bucket, r, name)
            assert all(abs(a[3] - e[3]) <= 1e-3 for a, e in zip(got[r][name], entries))
