"""float64 restatement of the learned head ensemble (include/scatten.h, sca_ensemble_log_probs_dw
and sca_ensemble_log_probs_dw_bwd) for tests/test_learned_ensemble.py and
tests/test_gpu_learned_ensemble.py, written from the header's formulas on top of
tests/ensemble_ref.py and tests/ensemble_grad_ref.py.  numpy only; no part of the package is used.

The weights are W = softmax(theta) of G unconstrained scores.  The forward and the members'
gradients are the host-weight ones with W.  With lp_g = log_softmax(x_g), q = exp(out) and
D = sum_c dout[c] per row, d theta (G) sums over all rows
  "prob":    s_g - W_g D,  s_g = sum_c r_g[c] dout[c],  r_g[c] = exp(lp_g[c] + log W_g - out[c])
  "logprob": W_g sum_c du[c] (lp_g[c] - out[c]),  du[c] = dout[c] - q[c] D
(out in the place of u = sum_g W_g lp_g is exact because sum_c du = 0)."""
import numpy as np

from tests import ensemble_grad_ref as GR
from tests import ensemble_ref as R


def softmax_weights(theta):
    t = np.asarray(theta, np.float64)
    assert t.ndim == 1 and np.isfinite(t).all()
    e = np.exp(t - t.max())
    return e / e.sum()


def theta_of(G):
    """The scores of the parity tests: the log of the unequal weights 0.2 / 1.0 / 3.0 cycled."""
    return np.log(np.asarray(R.cycled_weights(G), np.float64))


def ensemble(logits, theta, mode):
    """logits: G arrays (..., C); theta (G,).  The (..., C) float64 ensemble under softmax(theta)."""
    return R.ensemble(logits, softmax_weights(theta), mode)


def row_partials(logits, theta, mode, dout):
    """The (rows, G) float64 contributions of every row to d theta."""
    G, C = len(logits), np.asarray(logits[0]).shape[-1]
    w = softmax_weights(theta)
    dout = np.asarray(dout, np.float64).reshape(-1, C)
    lp = [R.log_softmax(x).reshape(-1, C) for x in logits]
    out = R.ensemble(logits, w, mode).reshape(-1, C)
    D = dout.sum(-1)
    res = np.zeros((dout.shape[0], G))
    for g in range(G):
        if mode == "prob":
            r = np.exp(lp[g] + np.log(w[g]) - out)
            res[:, g] = (r * dout).sum(-1) - w[g] * D
        else:
            assert mode == "logprob"
            du = dout - np.exp(out) * D[:, None]
            res[:, g] = w[g] * (du * (lp[g] - out)).sum(-1)
    return res


def dtheta(logits, theta, mode, dout):
    """d theta (G,) float64; exactly 0 for G = 1 (W = 1 whatever theta is)."""
    if len(logits) == 1:
        return np.zeros(1)
    return row_partials(logits, theta, mode, dout).sum(0)


def vjp(logits, theta, mode, dout):
    """(the G members' gradients, d theta): the members' as tests/ensemble_grad_ref.py gives them
    under W = softmax(theta)."""
    return GR.vjp(logits, softmax_weights(theta), mode, dout), dtheta(logits, theta, mode, dout)
