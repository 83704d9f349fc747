"""float64 restatement of sca_ensemble_log_probs_bwd (include/scatten.h), the vector-Jacobian
product of the head ensemble, for tests/test_ensemble_backward.py and
tests/test_gpu_ensemble_backward.py, written from the header's formulas on top of
tests/ensemble_ref.py.  numpy only; no part of the package is used.

Per row, p_g = softmax(x_g), lp_g = log p_g, W_g the normalised weight, q = exp(out):
  "prob":    r_g[c] = exp(lp_g[c] + log W_g - out[c])
             dx_g[k] = r_g[k] dout[k] - p_g[k] sum_c r_g[c] dout[c]
  "logprob": du[c] = dout[c] - q[c] sum_c' dout[c']
             dx_g[k] = W_g (du[k] - p_g[k] sum_c du[c])
The last sum is 0 analytically (sum q = 1); the restatement keeps the term, the kernel drops it."""
import numpy as np

from tests import ensemble_ref as R


def vjp(logits, weights, mode, dout):
    """logits: G arrays (..., C); dout (..., C).  Returns the G float64 gradients (..., C)."""
    G = len(logits)
    dout = np.asarray(dout, np.float64)
    lp = [R.log_softmax(x) for x in logits]
    w = R.normalised(weights, G)
    out = R.ensemble(logits, weights, mode)
    if mode == "prob":
        res = []
        for g in range(G):
            r = np.exp(lp[g] + np.log(w[g]) - out)
            res.append(r * dout - np.exp(lp[g]) * (r * dout).sum(-1, keepdims=True))
        return res
    assert mode == "logprob"
    du = dout - np.exp(out) * dout.sum(-1, keepdims=True)
    return [w[g] * (du - np.exp(lp[g]) * du.sum(-1, keepdims=True)) for g in range(G)]


def dout_of(shape, zero_rows=0):
    """The incoming gradient of the parity tests, (B, T, C) float32 of N(0, 1) from
    default_rng(7); the last `zero_rows` rows of the tensor are 0."""
    d = np.random.default_rng(7).standard_normal(tuple(shape)).astype(np.float32)
    if zero_rows:
        d.reshape(-1, shape[-1])[-zero_rows:] = 0.0
    return d
