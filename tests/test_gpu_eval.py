"""The evaluation step on the MI355X (scattennet_amd/evaluate.py; csrc/decode.hip: the grouped
decoders and sca_eval_accumulate): grouped against single-head decoding and the float64
restatement of tests/decode_ref.py, the accumulated state against sca_wer_counts and host sums,
the whole model on the reference's fixture, and capture / length buckets against the eager step.

As in tests/test_decode.py, equality of a discrete search only means something away from ties:
every beam case asserts on the CPU side that each head's inputs keep the restatement's gaps at
or above MIN_GAP.  That is a condition on the inputs (the seeds were chosen for it).

in_len is ragged and holds 0 and 1 wherever the case has the clips for it beside a full one
(B >= 3); the B = 2 case holds a 1, the B = 1 case is one full clip."""
import copy
import functools
import os

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests.golden_util import GOLDEN, close, load, load_arrays, rel_err

pytestmark = pytest.mark.gpu

MIN_GAP = 1e-4
TOL = 1e-3  # the project's relative bound
LOGITS = ["alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits"]
NAMES = ["alignment_", "left", "right", "body", "fuse_coord_"]  # the reference's logits_name of each
LOSSES = ["total_loss", "alignment_loss", "fuse_coord_loss", "left_distill_loss", "right_distill_loss",
          "body_distill_loss"]

# (B, T, C, W) -> (in_len, one seed per head)
CASES = {
    # G B T is no multiple of the 4 rows per top-k workgroup
    (3, 7, 5, 3): ([7, 0, 1], [1000, 1001, 1002, 1003, 1004]),
    # fewer labels than W + 1; pruned prefixes return
    (5, 16, 4, 8): ([16, 0, 1, 9, 16], [1000, 1001, 1002, 1003, 1005]),
    # odd sizes; beam 1 is not greedy
    (3, 37, 70, 1): ([37, 1, 0], [1000, 1001, 1002, 1003, 1004]),
    # the widest beam
    (2, 20, 33, 32): ([20, 1], [1001, 1003, 1005, 1006, 1007]),
    # 2241 arena nodes per clip, past the 2048 mirrored in LDS: a wrong per-head arena offset shows
    (1, 70, 6, 32): ([70], [1000, 1002, 1005, 1013, 1014]),
}
IDS = ["B%d_T%d_C%d_W%d" % s for s in CASES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _logits(shape, seed):
    B, T, C, _ = shape
    return np.random.default_rng(seed).normal(0.0, 4.0, (B, T, C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _beam_ref(shape, seed, collapse):
    """The restatement for one head of one case, computed once and shared."""
    return R.beam_search_batch(_logits(shape, seed), CASES[shape][0], shape[3], collapse)


def _rows(tokens, lengths):
    tokens, lengths = tokens.cpu().numpy(), lengths.cpu().numpy()
    return [tokens[b, :lengths[b]].tolist() for b in range(len(lengths))]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1: grouped decoding
@pytest.mark.parametrize("G", [1, 2, 5])
@pytest.mark.parametrize("shape", list(CASES), ids=IDS)
def test_grouped_beam_decode_equals_single_head_and_restatement(shape, G):
    import scattennet_amd as S
    dev = _dev()
    lens, seeds = CASES[shape]
    B, T, C, W = shape
    xs = [torch.from_numpy(_logits(shape, s)).to(dev) for s in seeds[:G]]
    il = torch.tensor(lens)
    for collapse in (True, False):
        tokens, lengths, scores = S.ctc_decode_heads_device(xs, il, beam_size=W, collapse_repeats=collapse)
        assert tokens.shape == (G, B, T) and lengths.shape == (G, B) and scores.shape == (G, B)
        assert tokens.dtype == torch.int32 and lengths.dtype == torch.int32 and scores.dtype == torch.float32
        for g in range(G):
            t1, l1, s1 = S.ctc_decode_device(xs[g], il, beam_size=W, collapse_repeats=collapse)
            assert torch.equal(tokens[g], t1) and torch.equal(lengths[g], l1), (g, collapse)
            assert torch.equal(_bits(scores[g]), _bits(s1)), (g, collapse)
            want, want_score, frame_gap, final_gap = _beam_ref(shape, seeds[g], collapse)
            assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP, (g, frame_gap, final_gap)  # on the inputs
            assert _rows(tokens[g], lengths[g]) == want, (g, collapse)
            assert rel_err(scores[g], torch.from_numpy(want_score)) < TOL
            assert not tokens[g].cpu().numpy()[np.arange(T)[None, :] >= l1.cpu().numpy()[:, None]].any()
    if G > 1:
        assert not torch.equal(tokens[0], tokens[1])  # the heads do differ


@pytest.mark.parametrize("G", [1, 2, 5])
@pytest.mark.parametrize("shape", list(CASES), ids=IDS)
def test_grouped_greedy_decode_equals_single_head_and_restatement(shape, G):
    import scattennet_amd as S
    dev = _dev()
    lens, seeds = CASES[shape]
    B, T, C, _ = shape
    xn = []
    for s in seeds[:G]:  # a small spread, blank boosts and repeated frames: blanks and repeats occur
        x = np.random.default_rng(s).normal(0.0, 1.0, (B, T, C)).astype(np.float32)
        x[:, :, 0] += 3.0 * (np.random.default_rng(s + 1).random((B, T)) < 0.3)
        for t in range(1, T, 3):
            x[:, t] = x[:, t - 1]
        xn.append(x)
    xs = [torch.from_numpy(x).to(dev) for x in xn]
    il = torch.tensor(lens)
    tokens, lengths, scores = S.ctc_decode_heads_device(xs, il, beam_size=0)
    assert tokens.shape == (G, B, T) and lengths.shape == (G, B)
    for g in range(G):
        t1, l1, s1 = S.ctc_greedy_decode_device(xs[g], il)
        assert torch.equal(tokens[g], t1) and torch.equal(lengths[g], l1) and torch.equal(_bits(scores[g]), _bits(s1))
        ref = [R.greedy(xn[g][b], lens[b]) for b in range(B)]
        assert _rows(tokens[g], lengths[g]) == [r[0] for r in ref], g
        assert rel_err(scores[g], torch.tensor([r[1] for r in ref])) < TOL


def test_grouped_decode_reduced_precision_logits_take_the_fp32_path():
    import scattennet_amd as S
    dev = _dev()
    shape = (3, 7, 5, 3)
    lens, seeds = CASES[shape]
    xs = [torch.from_numpy(_logits(shape, s)).to(dev).to(torch.bfloat16) for s in seeds[:2]]
    got = S.ctc_decode_heads_device(xs, torch.tensor(lens), beam_size=3)
    want = S.ctc_decode_heads_device([x.float() for x in xs], torch.tensor(lens), beam_size=3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert got[2].dtype == torch.bfloat16 and torch.equal(got[2], want[2].to(torch.bfloat16))


# ---------------------------------------------------------------- 2: accumulate
class _Stub:
    """What EvalState needs of a model: the distillation students and a parameter's device."""

    def __init__(self, dev, students=("left", "right", "body")):
        self._p = torch.nn.Parameter(torch.zeros(1, device=dev))
        self._s = list(students)

    def _students(self):
        return list(self._s)

    def parameters(self):
        return iter([self._p])


def _report(dev, nflags, losses, flags=None):
    """A finite_report as sca_step_report lays it out: flag words, the loss words, guard."""
    words = torch.zeros(nflags + len(losses) + 1, dtype=torch.int32)
    for i, f in (flags or {}).items():
        words[i] = f
    words[nflags:nflags + len(losses)] = torch.tensor(losses, dtype=torch.float32).view(torch.int32)
    return words.to(dev)


def _pairs(rng, N, width, vocab_of=lambda n: 2 + n % 7):
    """Random (reference, hypothesis) rows with few distinct tokens: many equal cells and ties."""
    rl, hl = rng.integers(0, width + 1, N), rng.integers(0, width + 1, N)
    ref, hyp = np.zeros((N, width), np.int32), np.zeros((N, width), np.int32)
    for n in range(N):
        ref[n, :rl[n]] = rng.integers(1, vocab_of(n) + 1, rl[n])
        hyp[n, :hl[n]] = rng.integers(1, vocab_of(n) + 1, hl[n])
    return ref, rl.astype(np.int32), hyp, hl.astype(np.int32)


def test_accumulate_counts_equal_wer_counts_on_tiled_references():
    import scattennet_amd as S
    from scattennet_amd import evaluate as E
    dev = _dev()
    with np.load(os.path.join(GOLDEN, "wer_cases.npz")) as z:
        fx = {k: z[k] for k in ("ref", "ref_len", "hyp", "hyp_len", "counts")}
    nf = len(fx["counts"])
    rng = np.random.default_rng(5)
    rr, rrl, rh, rhl = _pairs(rng, 18, 128)
    rrl[:4], rhl[:4] = [128, 0, 128, 1], [128, 128, 0, 127]  # the lengths 0 and 128
    for n in range(4):
        rr[n, :rrl[n]] = rng.integers(1, 4, rrl[n])
        rr[n, rrl[n]:] = 0
        rh[n, :rhl[n]] = rng.integers(1, 4, rhl[n])
        rh[n, rhl[n]:] = 0
    B, G = nf + 18, 2
    ref = np.zeros((B, 128), np.int32)
    ref[:nf, :fx["ref"].shape[1]] = fx["ref"]
    ref[nf:] = rr
    ref_len = np.concatenate([fx["ref_len"], rrl]).astype(np.int32)
    hyp0 = np.zeros((B, 128), np.int32)
    hyp0[:nf, :fx["hyp"].shape[1]] = fx["hyp"]
    hyp0[nf:] = rh
    len0 = np.concatenate([fx["hyp_len"], rhl]).astype(np.int32)
    tokens = np.stack([hyp0, np.roll(hyp0, 1, axis=0)])  # head 1: the hypotheses of the neighbouring clip
    lengths = np.stack([len0, np.roll(len0, 1)])
    state = S.EvalState(_Stub(dev))
    t, n = torch.from_numpy(tokens).to(dev), torch.from_numpy(lengths).to(dev)
    r, rn = torch.from_numpy(ref).to(dev), torch.from_numpy(ref_len).to(dev)
    counts = E.accumulate(state, t, n, r, rn, _report(dev, 15, [1.0] * 6))
    want = S.wer_counts(r.repeat(G, 1), rn.repeat(G), t.reshape(G * B, 128), n.reshape(-1)).reshape(G, B, 4)
    assert counts.dtype == torch.int32 and torch.equal(counts, want)
    assert counts[0, :nf].cpu().numpy().tolist() == fx["counts"].tolist()
    for g in range(G):
        for b in (nf, nf + 1, nf + 2, nf + 3, B - 1):
            assert tuple(counts[g, b].tolist()) == R.wer_single(ref[b, :ref_len[b]], tokens[g, b, :lengths[g, b]])
    raw = state.raw()
    assert raw["totals"][:G].tolist() == want.sum(1).tolist() and not raw["totals"][G:].any()
    assert raw["cursor"] == B and raw["steps"] == 1 and raw["overflow"] == 0 and raw["first_flagged"] == 0
    state.reset()
    raw = state.raw()
    assert raw["cursor"] == 0 and raw["steps"] == 0 and not raw["totals"].any() and not raw["loss_sum"].any()


def _three_batches(dev, B, width):
    rng = np.random.default_rng(17)
    out = []
    for _ in range(3):
        ref, rl, h0, l0 = _pairs(rng, B, width)
        _, _, h1, l1 = _pairs(rng, B, width)
        out.append(tuple(torch.from_numpy(a).to(dev) for a in (np.stack([h0, h1]), np.stack([l0, l1]), ref, rl)))
    return out


@pytest.mark.parametrize("short", [False, True], ids=["capacity_3B", "capacity_2B_plus_1"])
def test_accumulate_three_steps_totals_cursor_log_and_loss_sums(short):
    import scattennet_amd as S
    from scattennet_amd import evaluate as E
    dev = _dev()
    B, G, width = 4, 2, 9
    capacity = 2 * B + 1 if short else 3 * B
    state = S.EvalState(_Stub(dev), capacity=capacity, log_width=width)
    batches = _three_batches(dev, B, width)
    rng = np.random.default_rng(23)
    step_losses = [[float(v) for v in rng.uniform(0.05, 60.0, 6).astype(np.float32)] for _ in range(3)]
    reports = [_report(dev, 15, ls) for ls in step_losses]
    counts = [E.accumulate(state, t, n, r, rn, rep) for (t, n, r, rn), rep in zip(batches, reports)]
    raw = state.raw()
    assert raw["totals"][:G].tolist() == sum(c.sum(1) for c in counts).tolist()
    for (t, n, r, rn), c in zip(batches, counts):
        assert torch.equal(c, S.wer_counts(r.repeat(G, 1), rn.repeat(G), t.reshape(G * B, width),
                                           n.reshape(-1)).reshape(G, B, 4))
    assert raw["cursor"] == 3 * B and raw["steps"] == 3 and raw["first_flagged"] == 0
    # float64 sums in step order of the same float32 values the host reads with .item()
    host = [0.0] * 6
    for rep in reports:
        for i in range(6):
            host[i] += rep.view(torch.float32)[15 + i].item()
    assert raw["loss_sum"][:6].tolist() == host and not raw["loss_sum"][6:].any()
    # the log: clip b of step s is row s B + b, zero-padded; rows at or beyond capacity untouched
    log, log_len = state.hyp_log.cpu().numpy(), state.hyp_len_log.cpu().numpy()
    assert log.shape == (capacity, G, width)
    rows = 0
    for s, (t, n, _, _) in enumerate(batches):
        t, n = t.cpu().numpy(), n.cpu().numpy()
        for b in range(B):
            if s * B + b >= capacity:
                continue
            rows += 1
            for g in range(G):
                assert log_len[s * B + b, g] == n[g, b]
                assert log[s * B + b, g].tolist() == t[g, b, :n[g, b]].tolist() + [0] * (width - n[g, b])
    assert rows == capacity
    if short:  # the third call wrote one row and set the overflow bit; the totals are whole
        assert raw["overflow"] == 1
        with pytest.raises(RuntimeError, match="overflowed"):
            state.read()
        assert len(state.hypotheses()) == capacity
    else:
        assert raw["overflow"] == 0
        got = state.read()
        for i, k in enumerate(state.loss_names):
            assert got[k] == host[i] / 3
        hyps = state.hypotheses()
        assert len(hyps) == 3 * B and sorted(hyps[0]) == ["alignment_", "fuse_coord_"]
        t, n = batches[1][0].cpu().numpy(), batches[1][1].cpu().numpy()
        assert hyps[B + 2]["fuse_coord_"] == t[1, 2, :n[1, 2]].tolist()


def test_accumulate_flags_are_ored_and_the_first_flagged_step_is_kept():
    import scattennet_amd as S
    from scattennet_amd import evaluate as E
    dev = _dev()
    state = S.EvalState(_Stub(dev))
    batches = _three_batches(dev, 4, 9)
    flags = [None, {6: 1}, {0: 2, 6: 2}]
    for (t, n, r, rn), f in zip(batches, flags):
        E.accumulate(state, t, n, r, rn, _report(dev, 15, [1.0] * 6, f))
    raw = state.raw()
    assert raw["first_flagged"] == 2 and raw["flags"][0] == 2 and raw["flags"][6] == 3 and raw["steps"] == 3
    assert sum(raw["flags"]) == 5
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        state.read()


# ---------------------------------------------------------------- 3: the whole model
def _build(fx, dev):
    import scattennet_amd as S
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])), device="cuda")
    m.load_state_dict({k: v for k, v in fx["param"].items()}, strict=True)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def fx():
    return load("model_small", "manifest_model.json")


@pytest.fixture(scope="module")
def expected(fx):
    """decode_ref on the fixture's own reference logits, per mode and head, computed once; the
    gaps and the greedy top-2 margin are asserted here, on the CPU."""
    z = load_arrays("model_small")
    lens = fx["in"]["valid_len_in"].tolist()
    out = {}
    for beam in (5, 1):
        out[beam] = {}
        for k in LOGITS:
            hyps, _, frame_gap, final_gap = R.beam_search_batch(z["out." + k], lens, beam, True)
            assert frame_gap >= MIN_GAP and final_gap >= MIN_GAP, (beam, k, frame_gap, final_gap)
            out[beam][k] = hyps
    out[0] = {}
    for k in LOGITS:
        x = z["out." + k].astype(np.float64)
        for b, n in enumerate(lens):
            top = np.sort(x[b, :n], axis=-1)
            assert float((top[:, -1] - top[:, -2]).min()) >= MIN_GAP, (k, b)
        out[0][k] = [R.greedy(x[b], lens[b])[0] for b in range(len(lens))]
    return out


def _refs(fx):
    lab, n = fx["in"]["gloss_labels"].numpy(), fx["in"]["gloss_lengths"].tolist()
    return [lab[b, :n[b]].tolist() for b in range(len(n))]


def _src(fx, dev):
    return {k: v.to(dev) for k, v in fx["in"].items()}


@pytest.mark.parametrize("beam", [5, 1, 0], ids=["beam5", "beam1", "greedy"])
def test_eval_step_on_the_fixture_all_heads(fx, expected, beam):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    state = S.EvalState(model, heads=LOGITS, capacity=3, log_width=13)
    out = S.eval_step(model, _src(fx, dev), state, beam_size=beam)
    assert out["tokens"].shape == (5, 3, 13) and out["lengths"].shape == (5, 3) and out["counts"].shape == (5, 3, 4)
    assert model.training is False and model.check == "sync"
    hyps = state.hypotheses()
    assert len(hyps) == 3
    z = load_arrays("model_small")
    for g, k in enumerate(LOGITS):
        print(k, "logit rel err", rel_err(out[k], torch.from_numpy(z["out." + k])))
        for b in range(3):  # all 15 (head, clip) pairs
            assert hyps[b][NAMES[g]] == expected[beam][k][b], (k, b)
    got = state.read()
    refs = _refs(fx)
    rates = []
    for g, k in enumerate(LOGITS):
        want = R.wer_list(refs, expected[beam][k])["wer"]
        assert got[NAMES[g] + "wer"] == want, k
        rates.append(want)
    assert got["wer"] == min(rates + [200])
    for k in LOSSES:
        assert close(torch.tensor(got[k]), torch.from_numpy(z["out." + k]), TOL), (k, got[k], float(z["out." + k]))
    assert got["loss"] == got["total_loss"]


@pytest.mark.parametrize("beam", [5, 0], ids=["beam5", "greedy"])
def test_eval_step_is_the_composition_of_the_parts(fx, beam):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = _src(fx, dev)
    state = S.EvalState(model)  # the default heads: the two evaluate_fn decodes
    assert list(state.heads) == ["alignment_gloss_logits", "fuse_coord_gloss_logits"]
    out = S.eval_step(model, src, state, beam_size=beam)
    with torch.no_grad():
        plain = model(src)
    rep = S.read_report(plain)
    ref = src["gloss_labels"].to(torch.int32)
    total = torch.zeros(2, 4, dtype=torch.int64)
    for g, k in enumerate(state.heads):
        assert torch.equal(_bits(out[k]), _bits(plain[k]))
        if beam:
            t, n, _ = S.ctc_decode_device(plain[k], plain["input_lengths"], beam_size=beam)
        else:
            t, n, _ = S.ctc_greedy_decode_device(plain[k], plain["input_lengths"])
        c = S.wer_counts(ref, src["gloss_lengths"], t, n)
        assert torch.equal(out["tokens"][g], t) and torch.equal(out["lengths"][g], n)
        assert torch.equal(out["counts"][g], c)
        total[g] = c.sum(0).cpu()
    assert torch.equal(_bits(out["finite_report"]), _bits(plain["finite_report"]))
    got = state.read()
    for g, k in enumerate(state.heads):
        assert got[k.replace("gloss_logits", "") + "wer"] == S.wer_from_counts(total[g])["wer"]
    for k in LOSSES:
        assert got[k] == rep[k]  # one step: the float64 of the same float32
    # 1-D concatenated labels are split by the lengths
    flat = dict(src)
    flat["gloss_labels"] = torch.cat([fx["in"]["gloss_labels"][b, :n] for b, n in
                                      enumerate(fx["in"]["gloss_lengths"].tolist())])
    flat["gloss_lengths"] = fx["in"]["gloss_lengths"]
    flat["valid_len_in"] = fx["in"]["valid_len_in"]
    again = S.eval_step(model, flat, S.EvalState(model), beam_size=beam)
    assert torch.equal(again["counts"], out["counts"])


# ---------------------------------------------------------------- 4: capture and buckets
def _truncate(src, T):
    lens = src["mask"].sum(1).clamp(max=T)
    out = dict(src)
    out["keypoints"], out["mask"] = src["keypoints"][:, :T].contiguous(), src["mask"][:, :T].contiguous()
    out["valid_len_in"] = (lens >> 1).to(src["valid_len_in"].dtype)
    return out


def _same_state(a, b):
    ra, rb = a.raw(), b.raw()
    for k in ("cursor", "steps", "overflow", "first_flagged", "flags"):
        assert ra[k] == rb[k], k
    assert ra["totals"].tolist() == rb["totals"].tolist()
    assert ra["loss_sum"].tolist() == rb["loss_sum"].tolist()


def test_captured_eval_step_matches_three_eager_steps(fx):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    src = _src(fx, dev)
    eager = S.EvalState(model, capacity=9, log_width=13)
    for _ in range(3):
        S.eval_step(model, src, eager)
    state = S.EvalState(model, capacity=9, log_width=13)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.eval_step(model, src, state)  # the warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    state.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.eval_step(model, src, state)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    _same_state(state, eager)
    assert state.raw()["cursor"] == 9 and state.raw()["steps"] == 3
    assert state.hypotheses() == eager.hypotheses() and len(state.hypotheses()) == 9
    assert state.read() == eager.read()
    assert out["tokens"].shape == (2, 3, 13)


@pytest.fixture(scope="module")
def eager_steps(fx):
    """The unpadded eager eval_step of the fixture batch (T = 26) and of its 21-frame cut: the
    step's hypotheses, counts and losses, computed once."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    full = _src(fx, dev)
    out = {}
    for T, src in ((26, full), (21, _truncate(full, 21)), (2, {k: v[:2].contiguous() for k, v in full.items()})):
        state = S.EvalState(model, capacity=3, log_width=13)
        o = S.eval_step(model, src, state)
        out[T] = {"hyps": state.hypotheses(), "counts": o["counts"].cpu(), "read": state.read(),
                  "totals": state.raw()["totals"]}
    return out


def _rows2(tokens, lengths):
    """(2, B, T) tokens -> per clip {logits_name: ids} for the two default heads."""
    t, n = tokens.cpu().numpy(), lengths.cpu().numpy()
    return [{name: t[g, b, :n[g, b]].tolist() for g, name in enumerate(("alignment_", "fuse_coord_"))}
            for b in range(t.shape[1])]


def _check_step(out, want, T, label):
    assert out["tokens"].shape == (2, 3, T >> 1) and out["fuse_coord_gloss_logits"].shape[1] == T >> 1, label
    assert torch.equal(out["counts"].cpu(), want["counts"]), label
    assert _rows2(out["tokens"], out["lengths"]) == want["hyps"], label


@pytest.mark.parametrize("bucket,T", [(28, 26), (32, 26), (40, 26), (32, 21)])
def test_bucketed_eval_step_matches_the_unpadded_eager_step(fx, eager_steps, bucket, T):
    """Three feeds: the eager, the capture and the replay path of the bucket."""
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    full = _src(fx, dev)
    src = full if T == 26 else _truncate(full, T)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(bucket,), label_bucket=3, capacity=9)
    assert bes.state.log_width == bucket >> 1 and bes.bucket_for(T) == bucket
    want = eager_steps[T]
    captured = []
    for i in range(3):
        _check_step(bes.step(src), want, T, (bucket, T, i))
        captured.append(bes.graphs_captured)
    assert captured == [0, 1, 1] and bes._buckets[bucket].uses == 3 and bes.eager_fallbacks == 0
    raw = bes.state.raw()
    assert raw["totals"].tolist() == (3 * want["totals"]).tolist() and raw["cursor"] == 9 and raw["steps"] == 3
    assert bes.hypotheses() == want["hyps"] * 3
    got = bes.read()
    for k in LOSSES:
        print(f"bucket {bucket} T {T}: {k} {got[k]:.7g} unpadded {want['read'][k]:.7g}")
        assert abs(got[k] - want["read"][k]) < TOL * abs(want["read"][k]), k
    for k in ("alignment_wer", "fuse_coord_wer", "wer"):
        assert got[k] == want["read"][k], k


def test_bucketed_eval_step_buckets_share_one_state(fx, eager_steps):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    full = _src(fx, dev)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        S.BucketedEvalStep(model, 3, (28, 128), 3)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(24, 32), label_bucket=3, capacity=32)
    srcs = {26: full, 21: _truncate(full, 21), 2: {k: v[:2].contiguous() for k, v in full.items()}}
    order = (21, 26, 21, 26, 21, 26)
    for i, T in enumerate(order):
        _check_step(bes.step(srcs[T]), eager_steps[T], T, i)
    assert bes.graphs_captured == 2 and [bes._buckets[f].uses for f in (24, 32)] == [3, 3]
    # a batch of two clips takes the eager path and still accumulates
    out = bes.step(srcs[2])
    assert bes.eager_fallbacks == 1 and out["tokens"].shape == (2, 2, 13) and bes.graphs_captured == 2
    assert torch.equal(out["counts"].cpu(), eager_steps[2]["counts"])
    raw = bes.state.raw()
    assert raw["cursor"] == 20 and raw["steps"] == 7 and raw["overflow"] == 0
    want = sum(eager_steps[T]["totals"] for T in order + (2,))
    assert raw["totals"].tolist() == want.tolist()
    assert bes.hypotheses() == sum((eager_steps[T]["hyps"] for T in order + (2,)), [])
    got = bes.read()
    assert got["fuse_coord_wer"] == S.wer_from_counts(torch.from_numpy(want[1:2].astype(np.int64)))["wer"]
    mean = sum(eager_steps[T]["read"]["total_loss"] for T in order + (2,)) / 7
    assert abs(got["loss"] - mean) < TOL * abs(mean)


def test_bucketed_eval_step_nan_keeps_the_clean_totals(fx, eager_steps):
    import scattennet_amd as S
    dev = _dev()
    model = _build(fx, dev)
    full = _src(fx, dev)
    bes = S.BucketedEvalStep(model, batch_size=3, frame_buckets=(32,), label_bucket=3)
    for _ in range(2):
        bes.step(full)
    assert bes.graphs_captured == 1
    clean = bes.state.raw()["totals"].copy()
    assert clean[:2].tolist() == (2 * eager_steps[26]["totals"][:2]).tolist()
    bad = dict(full)
    bad["keypoints"] = full["keypoints"].clone()
    bad["keypoints"][1, 3, 6, 0] = float("nan")  # a valid frame of clip 1
    bes.step(bad)  # a replay
    raw = bes.state.raw()
    assert raw["first_flagged"] == 3 and raw["steps"] == 3 and raw["flags"][0] == 1
    with pytest.raises(ValueError, match="NaN or inf in input keypoints"):
        bes.read()
    # the clean steps' totals are still there: the flagged step added its own counts on top
    assert (raw["totals"][:2, 3] == 3 * eager_steps[26]["totals"][:2, 3]).all()  # num_ref: not from the logits
    assert (raw["totals"][:2, :3] >= clean[:2, :3]).all()
