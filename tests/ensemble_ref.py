"""float64 restatement of sca_ensemble_log_probs (include/scatten.h) for tests/test_ensemble.py
and tests/test_gpu_ensemble.py, written from the header's formulas.  The reference project has
no ensemble, so this restatement is the yardstick.  numpy only; no part of the package is used.

Also the inputs both test files share: `case` (random logits with the clamp rows) and the beam
case whose tie margins the CPU file checks and the GPU file decodes."""
import numpy as np

MODES = ("prob", "logprob")


def log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


def normalised(weights, G):
    w = np.full(G, 1.0) if weights is None else np.asarray(weights, np.float64)
    assert w.shape == (G,) and np.isfinite(w).all() and (w > 0).all()
    return w / w.sum()


def ensemble(logits, weights=None, mode="prob"):
    """logits: G arrays (..., C).  Returns the (..., C) float64 ensemble of the header."""
    lp = [log_softmax(x) for x in logits]
    w = normalised(weights, len(lp))
    if mode == "prob":  # out = M + log sum_g exp(a_g - M), a_g = lp_g + log w_g, M = max_g a_g
        a = np.stack([lp[g] + np.log(w[g]) for g in range(len(lp))])
        M = a.max(0)
        return M + np.log(np.exp(a - M).sum(0))
    assert mode == "logprob"
    u = np.zeros_like(lp[0])
    for g in range(len(lp)):  # g ascending
        u = u + w[g] * lp[g]
    return log_softmax(u)


def cycled_weights(G):
    """The unequal weights of the parity tests: 0.2 / 1.0 / 3.0 cycled."""
    return [(0.2, 1.0, 3.0)[g % 3] for g in range(G)]


def case(G, B, T, C, seed=0, clamp_rows=False):
    """G fp32 arrays (B, T, C) of 3 N(0, 1).  clamp_rows (needs G >= 2, B T >= 3, C >= 2): row 0
    has member 0 at +50 on class 1 where member 1 holds -50, row 1 the other way round on class
    0, and in row 2 every member is at -50 except on class C - 1."""
    rng = np.random.default_rng(1000 * G + 100 * B + 10 * T + C + seed)
    xs = [(3.0 * rng.standard_normal((B, T, C))).astype(np.float32) for _ in range(G)]
    if clamp_rows:
        assert G >= 2 and B * T >= 3 and C >= 2
        flat = [x.reshape(B * T, C) for x in xs]  # views
        flat[0][0, 1], flat[1][0, 1] = 50.0, -50.0
        flat[0][1, 0], flat[1][1, 0] = -50.0, 50.0
        for f in flat:
            f[2, :] = -50.0
            f[2, C - 1] = 1.5
    return xs


# the beam-decode case: (G, B, T, C) = (2, 3, 16, 8), beam 5; the seed is checked on the CPU
# (tests/test_ensemble.py) to keep decode_ref's tie margins above 1e-4 in both modes
BEAM_SHAPE, BEAM_WIDTH, BEAM_SEED = (2, 3, 16, 8), 5, 0
BEAM_LENS = (16, 11, 16)


def beam_case():
    return case(*BEAM_SHAPE, seed=BEAM_SEED)
