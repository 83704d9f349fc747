"""Float64 numpy restatement of CTC forced alignment as include/scatten.h states it
(sca_ctc_align_heads), word for word including the tie rules.  Uses nothing from the package.

`align(x, T_b, labels)` for one clip: x (T, C) logits, T_b valid frames, labels a sequence of
class ids in [1, C).  Returns (score, path, frame_label, spans, conf, gap):

  score        the path's log-probability (-inf: infeasible; 0.0 for T_b = 0 and no labels)
  path         the class emitted at every frame t < T_b (0 = blank), None when infeasible
  frame_label  (T,) int: the label INDEX j at frame t, -1 at blanks and at t >= T_b
  spans        (S, 2) int: [start, end) of label j
  conf         (S,) float64: mean over the span of exp(lp_t[l_j])
  gap          the smallest difference between the best and the second-best predecessor over the
               decisions on the returned path, and of the end choice (inf when there was never
               a second candidate): how far the path is from a tie
"""
import numpy as np

NEG_INF = -np.inf


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def align(x, T_b, labels):
    x = np.asarray(x, dtype=np.float64)
    T = x.shape[0]
    labels = [int(c) for c in labels]
    S_b = len(labels)
    T_b = min(max(int(T_b), 0), T)
    L = 2 * S_b + 1
    frame_label = np.full(T, -1, dtype=np.int64)
    spans = np.zeros((S_b, 2), dtype=np.int64)
    conf = np.zeros(S_b, dtype=np.float64)
    if T_b == 0:
        if S_b == 0:
            return 0.0, [], frame_label, spans, conf, np.inf
        return NEG_INF, None, frame_label, spans, conf, np.inf
    lp = log_softmax(x[:T_b])
    ext = [0 if s % 2 == 0 else labels[s // 2] for s in range(L)]
    v = np.full((T_b, L), NEG_INF)
    back = np.zeros((T_b, L), dtype=np.int64)
    margin = np.full((T_b, L), np.inf)  # best minus second-best predecessor of the decision at (t, s)
    v[0, 0] = lp[0, 0]
    if L > 1:
        v[0, 1] = lp[0, ext[1]]
    ext_a = np.array(ext)
    # the third term: odd s >= 3 whose label differs from the label at s - 2
    skip = np.zeros(L, dtype=bool)
    skip[3::2] = ext_a[3::2] != ext_a[1:-2:2]
    for t in range(1, T_b):  # all states s of frame t at once
        stay = v[t - 1]
        one = np.concatenate([[NEG_INF], stay])[:L]                             # v[t-1, s-1], s >= 1
        two = np.where(skip, np.concatenate([[NEG_INF] * 2, stay])[:L], NEG_INF)  # v[t-1, s-2] where allowed
        # the predecessor is s unless s - 1 is strictly greater; s - 2 only if strictly
        # greater than both
        best, k = stay.copy(), np.zeros(L, dtype=np.int64)
        take = one > best
        best, k = np.where(take, one, best), np.where(take, 1, k)
        take = two > best
        best, k = np.where(take, two, best), np.where(take, 2, k)
        v[t] = lp[t, ext_a] + best
        back[t] = k
        second = np.sort(np.stack([stay, one, two]), axis=0)[1]
        with np.errstate(invalid="ignore"):
            margin[t] = np.where(best > NEG_INF, best - second, np.inf)  # inf when the runner-up is -inf
    # the end state is L - 1 only if v[L - 1] > v[L - 2], otherwise L - 2; L = 1 ends in state 0
    if L == 1:
        end, gap = 0, np.inf
    else:
        a, b = v[T_b - 1, L - 1], v[T_b - 1, L - 2]
        end = L - 1 if a > b else L - 2
        gap = abs(a - b) if max(a, b) > NEG_INF else np.inf
    score = v[T_b - 1, end]
    if score == NEG_INF:
        return NEG_INF, None, frame_label, spans, conf, np.inf
    states = [0] * T_b
    s = end
    for t in range(T_b - 1, -1, -1):
        states[t] = s
        if t > 0:
            gap = min(gap, margin[t, s])
            s -= back[t, s]
    path = [ext[s] for s in states]
    for t, s in enumerate(states):
        if s % 2 == 1:
            frame_label[t] = s // 2
    for j in range(S_b):
        frames = np.nonzero(frame_label[:T_b] == j)[0]
        spans[j] = (frames[0], frames[-1] + 1)
        conf[j] = np.exp(lp[frames[0]:frames[-1] + 1, labels[j]]).mean()
    return float(score), path, frame_label, spans, conf, float(gap)


def collapse(path):
    """The CTC collapse of a frame-wise class path: merge repeats, drop blanks."""
    out, prev = [], None
    for c in path:
        if c != prev and c != 0:
            out.append(int(c))
        prev = c
    return out


def path_logprob(x, path):
    """Float64 log-probability of a frame-wise class path under log_softmax(x)."""
    lp = log_softmax(np.asarray(x, dtype=np.float64)[:len(path)])
    return float(sum(lp[t, c] for t, c in enumerate(path)))


def needed_frames(labels):
    """The fewest frames that can emit `labels`: their count plus the adjacent equal pairs."""
    labels = list(labels)
    return len(labels) + sum(1 for a, b in zip(labels, labels[1:]) if a == b)
