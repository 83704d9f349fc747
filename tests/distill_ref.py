"""float64 restatement of sca_distill_heads_fwd / _bwd (include/scatten.h) for
tests/test_ensemble_distill.py and tests/test_gpu_ensemble_distill.py: by definition the
composition of the two restatements the project already has,
    oracle.heads_oracle.seqkd(student, tests.ensemble_ref.ensemble(members, weights, mode), ...).
numpy only; no part of the package is used.  Also the inputs both test files share."""
import numpy as np

from oracle import heads_oracle as HO
from tests import ensemble_ref as R

# (G, S, B, T, C, start, temp): the parity cases
CASES = [(1, 1, 1, 1, 2, 1, 1.0),      # one column left: loss and gradients are exactly 0
         (2, 1, 1, 5, 7, 1, 1.0),      # rows not a multiple of 4, odd C < 64, scalar path
         (3, 2, 2, 4, 260, 1, 0.5),    # vector path, the first pack straddles `start`
         (8, 8, 1, 3, 130, 0, 2.0),    # largest G and S, blank included, C = 2 * 64 + 2
         (5, 3, 2, 9, 1124, 1, 1.0)]   # the vocabulary width
IDS = ["G%d_S%d_B%d_T%d_C%d_start%d_temp%g" % c for c in CASES]


def distill(students, members, student_weights, weights=None, mode="prob", temp=1.0, use_blank=False, lo=-100.0,
            hi=100.0):
    """-> (losses (S,), [d loss_s / d student_s]), float64.  The teacher is detached."""
    e = R.ensemble(members, weights, mode)
    out = [HO.seqkd(s, e, w, temp, use_blank, lo, hi) for s, w in zip(students, student_weights)]
    return np.array([o[0] for o in out]), [o[1] for o in out]


def case(G, S, B, T, C, seed=0, clamp_rows=False):
    """(students, members): S + G fp32 arrays (B, T, C) of 3 N(0, 1); the members are
    ensemble_ref.case's (with its rows at the heads' clamp when asked)."""
    members = R.case(G, B, T, C, seed=seed, clamp_rows=clamp_rows)
    rng = np.random.default_rng(77 + 1000 * S + 100 * B + 10 * T + C + seed)
    students = [(3.0 * rng.standard_normal((B, T, C))).astype(np.float32) for _ in range(S)]
    return students, members
