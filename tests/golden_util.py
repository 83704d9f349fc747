"""Loading helpers for the committed golden fixtures (tests/golden/*.npz)."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def manifest(fname="manifest.json"):
    with open(os.path.join(GOLDEN, fname)) as f:
        return json.load(f)


PART_BYTES = 900 * 1024  # array bytes per file: every committed fixture file stays under 1 MiB


def save_parts(name, arrs, directory=GOLDEN):
    """Write the arrays of one fixture as <name>.npz and, when they do not fit in PART_BYTES,
    the rest as <name>.part2.npz, <name>.part3.npz, ... (keys in order, each array whole)."""
    parts, size = [{}], 0
    for k, v in arrs.items():
        v = np.asarray(v)
        if parts[-1] and size + v.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = v
        size += v.nbytes
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(directory, name + (f".part{i + 1}" if i else "") + ".npz"), **part)
    return len(parts)


def load_arrays(name):
    """Every array of fixture `name`, from <name>.npz and its .partN.npz continuations."""
    z, i = {}, 1
    path = os.path.join(GOLDEN, name + ".npz")
    while os.path.exists(path):
        with np.load(path) as f:  # allow_pickle=False (default)
            z.update({k: f[k] for k in f.files})
        i += 1
        path = os.path.join(GOLDEN, f"{name}.part{i}.npz")
    if not z:
        raise FileNotFoundError(os.path.join(GOLDEN, name + ".npz"))
    return z


def load(name, manifest_name="manifest.json"):
    z = load_arrays(name)
    fx = {"in": {}, "param": {}, "grad_in": {}, "grad_param": {}}
    for k in z:
        v = torch.from_numpy(z[k].copy())
        if k.startswith("in."):
            fx["in"][k[3:]] = v
        elif k.startswith("param."):
            fx["param"][k[6:]] = v
        elif k.startswith("grad.in."):
            fx["grad_in"][k[8:]] = v
        elif k.startswith("grad.param."):
            fx["grad_param"][k[11:]] = v
        else:
            fx[k] = v
    fx["meta"] = manifest(manifest_name)["fixtures"][name]
    return fx


def rel_err(a, b):
    """max |a-b| / max(|b|, floor) — the 'relative fp32' metric used by every parity test."""
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    scale = b.abs().max().clamp_min(1e-6)
    return float((a - b).abs().max() / scale)


def close(a, b, tol, gscale=None, noise=1e-4):
    """Parity predicate.  `rel_err(a, b) < tol`, except for tensors that are analytically
    zero in the reference (e.g. the key-projection bias gradient: softmax is invariant to
    a per-row constant, so d/d(bk) is pure rounding noise): when |b| is below 1e-4 of the
    fixture's gradient scale `gscale`, both sides only have to be noise-level (< 1e-4 gscale;
    `noise`: that fraction for reduced-precision fixtures, whose rounding noise is larger)."""
    if gscale is not None:
        bmax = float(b.detach().abs().max()) if b.numel() else 0.0
        if bmax < noise * gscale:
            amax = float(a.detach().abs().max()) if a.numel() else 0.0
            return amax < noise * gscale
    return rel_err(a, b) < tol
