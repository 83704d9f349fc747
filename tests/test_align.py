"""CTC forced alignment, the parts that need no GPU: the float64 restatement of
tests/align_ref.py checked against an enumeration of every path, the host conversion
`alignment_lists`, and the validation that runs before the device check.  CPU only."""
import itertools

import numpy as np
import pytest
import torch

from tests import align_ref as R


# ------------------------------------------------------------- the restatement, by enumeration
def _enumerate(x, T_b, labels):
    """(best log-probability, the set of best paths, number of paths) over all C^T_b frame-wise
    class paths that collapse to `labels`."""
    C = x.shape[1]
    lp = R.log_softmax(x[:T_b])
    best, argbest, n = -np.inf, [], 0
    for path in itertools.product(range(C), repeat=T_b):
        if R.collapse(path) != list(labels):
            continue
        n += 1
        val = float(sum(lp[t, c] for t, c in enumerate(path)))
        if val > best + 1e-12:
            best, argbest = val, [list(path)]
        elif abs(val - best) <= 1e-12:
            argbest.append(list(path))
    return best, argbest, n


def test_restatement_equals_the_enumeration_of_all_paths():
    rng = np.random.default_rng(0)
    cases = 0
    for T in range(1, 6):
        for C in (2, 3):
            for S in range(0, 3):
                for labels in itertools.product(range(1, C), repeat=S):
                    x = rng.normal(0.0, 3.0, (T, C))
                    for T_b in range(0, T + 1):
                        score, path, frame_label, spans, conf, gap = R.align(x, T_b, labels)
                        want, paths, n = _enumerate(x, T_b, labels)
                        cases += 1
                        if T_b < R.needed_frames(labels) or (T_b == 0 and S > 0):
                            assert n == 0 and score == -np.inf and path is None
                            assert (frame_label == -1).all() and not spans.any() and not conf.any()
                            continue
                        assert n > 0 and abs(score - want) < 1e-9, (T, C, labels, T_b)
                        assert path in paths
                        assert R.collapse(path) == list(labels) and len(path) == T_b
                        assert abs(R.path_logprob(x, path) - score) < 1e-9
                        assert gap >= 0
                        # spans, frame_label and conf describe that path
                        lp = R.log_softmax(x[:T_b]) if T_b else None
                        for j, c in enumerate(labels):
                            s, e = spans[j]
                            assert e > s and all(path[t] == c for t in range(s, e))
                            assert (frame_label[s:e] == j).all()
                            assert abs(conf[j] - np.exp(lp[s:e, c]).mean()) < 1e-12
                        assert (frame_label[T_b:] == -1).all()
                        assert [t for t in range(T_b) if frame_label[t] < 0] == [t for t in range(T_b) if path[t] == 0]
    assert cases == 200


def test_restatement_tie_rules_on_equal_logits():
    """All-equal logits: every path ties, so the result is decided by the tie rules alone: the
    path ends in the last label's state rather than the final blank, and the walk back stays in a
    state for as long as that state was reachable, so the last label is held from the earliest
    frame that can reach it."""
    score, path, frame_label, spans, conf, gap = R.align(np.zeros((9, 4)), 9, [1, 2, 3])
    assert gap == 0.0
    assert abs(score - 9 * np.log(0.25)) < 1e-12
    assert path == [1, 2, 3, 3, 3, 3, 3, 3, 3]
    assert spans.tolist() == [[0, 1], [1, 2], [2, 9]]
    assert np.allclose(conf, 0.25)
    score, path, _, spans, _, _ = R.align(np.zeros((5, 3)), 5, [1, 1])  # a repeat needs its blank
    assert path == [1, 0, 1, 1, 1] and spans.tolist() == [[0, 1], [2, 5]]


# ------------------------------------------------------------------------- alignment_lists
def test_alignment_lists_conversions():
    import scattennet_amd as S
    labels = np.array([[5, 7, 5], [9, 0, 0], [3, 4, 0], [0, 0, 0]])
    n = np.array([3, 1, 2, 0])
    spans = np.array([[[0, 2], [2, 3], [5, 9]], [[4, 6], [0, 0], [0, 0]], [[0, 0], [0, 0], [0, 0]],
                      [[0, 0], [0, 0], [0, 0]]])
    conf = np.array([[0.5, 0.25, 1.0], [0.125, 0, 0], [0, 0, 0], [0, 0, 0]], dtype=np.float32)
    scores = np.array([-3.5, -1.0, -np.inf, -0.25], dtype=np.float32)
    got = S.alignment_lists(labels, n, spans, conf, scores)
    assert got == [[(5, 0, 2, 0.5), (7, 2, 3, 0.25), (5, 5, 9, 1.0)], [(9, 4, 6, 0.125)], None, []]
    assert all(type(v) is int for v in got[0][0][:3]) and type(got[0][0][3]) is float
    scaled = S.alignment_lists(labels, n, spans, conf, scores, frame_scale=4)
    assert scaled[0] == [(5, 0, 8, 0.5), (7, 8, 12, 0.25), (5, 20, 36, 1.0)] and scaled[2] is None and scaled[3] == []
    # torch tensors are taken as they are
    assert S.alignment_lists(torch.from_numpy(labels), torch.from_numpy(n), torch.from_numpy(spans),
                             torch.from_numpy(conf), torch.from_numpy(scores)) == got


# ------------------------------------------------------------------------------ validation
def test_validation_errors_come_before_the_device_check():
    import scattennet_amd as S
    x = torch.zeros(2, 6, 5)
    il, lab, n = torch.tensor([6, 4]), torch.tensor([[1, 2, 3], [4, 1, 1]]), torch.tensor([3, 1])
    with pytest.raises(RuntimeError, match=r"\(B, T, C\)"):
        S.ctc_align_device(torch.zeros(6, 5), il, lab, n)
    with pytest.raises(RuntimeError, match=r"\(B, T, C\)"):
        S.ctc_align_heads_device([x, torch.zeros(2, 6)], il, lab, n)
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.ctc_align_heads_device([], il, lab, n)
    with pytest.raises(ValueError, match="same shape"):
        S.ctc_align_heads_device([x, torch.zeros(2, 6, 4)], il, lab, n)
    with pytest.raises(RuntimeError, match="at most 6"):
        S.ctc_align_device(x, torch.tensor([7, 4]), lab, n)
    with pytest.raises(RuntimeError, match="to have 2 entries"):
        S.ctc_align_device(x, torch.tensor([6, 4, 1]), lab, n)
    with pytest.raises(RuntimeError, match="label_lengths to have value at most 3"):
        S.ctc_align_device(x, il, lab, torch.tensor([4, 1]))
    with pytest.raises(RuntimeError, match="non-negative"):
        S.ctc_align_device(x, il, lab, torch.tensor([3, -1]))
    with pytest.raises(RuntimeError, match="label_lengths to have 2 entries"):
        S.ctc_align_device(x, il, lab, torch.tensor([3]))
    with pytest.raises(RuntimeError, match=r"labels must be \(B, S\)"):
        S.ctc_align_device(x, il, torch.tensor([1, 2, 3]), n)
    with pytest.raises(RuntimeError, match="labels must be"):
        S.ctc_align_heads_device([x, x], il, lab.expand(3, 2, 3), torch.tensor([[3, 1]] * 3))
    with pytest.raises(ValueError, match=r"\[1, 5\)"):  # the blank inside the length
        S.ctc_align_device(x, il, torch.tensor([[1, 0, 3], [4, 1, 1]]), n)
    with pytest.raises(ValueError, match=r"\[1, 5\)"):
        S.ctc_align_device(x, il, torch.tensor([[1, 2, 5], [4, 1, 1]]), n)
    with pytest.raises(ValueError, match="exceed the kernel's 1023"):
        S.ctc_align_device(x, il, torch.ones(2, 1024, dtype=torch.long), n)
    # values outside the lengths are padding and pass; what is left is the device check
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_align_device(x, il, torch.tensor([[1, 2, 3], [4, 0, 99]]), n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_align_heads_device([x, x], il, lab.expand(2, 2, 3), torch.tensor([[3, 1], [0, 3]]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_align(x, il, lab, n)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.align_outputs({"fuse_coord_gloss_logits": x, "alignment_gloss_logits": x, "input_lengths": il}, lab, n)


class _Stub:
    def __init__(self):
        self._p = torch.nn.Parameter(torch.zeros(1))

    def _students(self):
        return ["left", "right", "body"]

    def parameters(self):
        return iter([self._p])


def test_eval_state_align_needs_a_log():
    import scattennet_amd as S
    with pytest.raises(ValueError, match="align=True needs a log"):
        S.EvalState(_Stub(), align=True, capacity=0)
    with pytest.raises(ValueError, match="align=True needs a log"):
        S.EvalState(_Stub(), align=True)
    state = S.EvalState(_Stub(), capacity=4, log_width=6, align=True)
    assert state.align and state.span_log.shape == (4, 2, 6, 2) and state.conf_log.shape == (4, 2, 6)
    assert state.score_log.shape == (4, 2) and state.span_log.dtype == torch.int32
    plain = S.EvalState(_Stub(), capacity=4, log_width=6)
    assert not plain.align and plain.span_log is None and plain.conf_log is None and plain.score_log is None
    with pytest.raises(RuntimeError, match="without align=True"):
        plain.alignments()
