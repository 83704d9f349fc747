"""Generate the whole-model golden fixture from the REFERENCE implementation.

Runs ONLY in the build container, where `/root/reference` (tinh2044/SCAttenNet, snapshot
2025-07-18) is importable; the outputs (data only: inputs, weights, outputs, gradients,
recorded losses) are committed as `model_small*.npz` + `manifest_model.json`.

* `model_small`: the reference `MSCA_Net` (model/__init__.py:72-290) in eval() at the smallest
  config that still walks every path (three streams, one pool, fusion, four classifiers, the
  BiLSTM alignment head, two CTC losses, three SeqKD terms): inputs, the whole state_dict,
  every output, every parameter gradient of `total_loss`.
* `model_train_steps` (arrays `train.*` of the same files): the reference's own loop
  (opt.py:28-38) for six steps on that batch with torch.optim.Adam(lr 2e-3, betas (0.9, 0.998),
  weight_decay 2e-5) and clip 1.0.  Stated deviation: the model stays in eval(), so dropout
  is off (the reference trains in train(), whose masks cannot be reproduced).  An fp64 copy
  of the reference runs the same loop; its distance from the fp32 trajectory is the floor
  the manifest records.

The generator asserts the conditions the parity tests rest on (losses below their clamps,
logits strictly inside +-50, per-sample CTC losses finite) and records them in the manifest.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_model.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

from model import MSCA_Net  # noqa: E402  (the reference's)

from scattennet_amd import workloads as W  # noqa: E402  (cfg helper only)
from tests.golden_util import save_parts  # noqa: E402

STEPS = 6
ADAM = dict(lr=2e-3, betas=(0.9, 0.998), weight_decay=2e-5)
CLIP = 1.0


def small_cfg():
    cfg = W.model_cfg(64, 4, layers=1, ff_mult=2, maxpos=64, residual_blocks=[64, 64])
    cfg.update({"body_idx": [1, 2, 3], "left_idx": list(range(5, 10)), "right_idx": list(range(10, 15)),
                "in_fusion_dim": 64, "out_fusion_dim": 64, "num_frame": 26, "self_distillation": True,
                "distillation_weight": {"left": 1.0, "right": 0.5, "body": 0.25},
                "alignment_module": {"input_size": 64, "hidden_size": 32, "num_layers": 2, "dropout": 0.3,
                                     "bidirectional": True}})
    return cfg


def batch():
    B, T, K = 3, 26, 16
    lengths = torch.tensor([26, 17, 12])
    kp = torch.rand(B, T, K, 2, generator=torch.Generator().manual_seed(0))
    mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lengths.tolist()):
        mask[b, :n] = 1
        kp[b, n:] = 0
    return {"keypoints": kp, "mask": mask, "valid_len_in": lengths // 2,  # one pool leaves 13 frames
            "gloss_labels": torch.tensor([[3, 4, 5], [2, 2, 1], [7, 1, 1]]), "gloss_lengths": torch.tensor([3, 2, 1])}


def train(model, src, dtype):
    model = copy.deepcopy(model).to(dtype).eval()
    src = {k: v.to(dtype) if v.is_floating_point() else v for k, v in src.items()}
    opt = torch.optim.Adam(model.parameters(), **ADAM)
    losses, norms = [], []
    for _ in range(STEPS):  # opt.py:28-38
        opt.zero_grad()
        out = model(src)
        loss = out["total_loss"]
        assert not (torch.isnan(loss) or torch.isinf(loss))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=CLIP)))
        opt.step()
        model.zero_grad()
        losses.append(float(loss))
    return np.array(losses, np.float64), np.array(norms, np.float64)


def main():
    torch.manual_seed(0)
    cfg = small_cfg()
    vocab = 12
    model = MSCA_Net(copy.deepcopy(cfg), list(range(vocab)), device="cpu").eval()
    src = batch()
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}

    out = model(src)
    out["total_loss"].backward()
    arrs = {}
    for k, v in src.items():
        arrs["in." + k] = v.numpy().astype(np.float32 if v.is_floating_point() else np.int64)
    for k, v in state.items():
        arrs["param." + k] = v.numpy()
    for k, v in out.items():
        arrs["out." + k] = v.detach().numpy()
    no_grad = []
    for k, p in model.named_parameters():
        if p.grad is None:
            no_grad.append(k)
        else:
            arrs["grad.param." + k] = p.grad.numpy()

    # the conditions the parity tests rest on
    logit_keys = ["alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits"]
    max_logit = max(float(out[k].detach().abs().max()) for k in logit_keys)
    assert max_logit < 50.0, max_logit
    losses = {k: float(v) for k, v in out.items() if "loss" in k and "gloss" not in k}
    assert all(0.0 < losses[k] < 100.0 for k in ("alignment_loss", "fuse_coord_loss")), losses
    assert all(abs(losses[k]) < 100.0 for k in losses if k.endswith("distill_loss")), losses
    per_sample = {}
    for k in ("alignment_gloss_logits", "fuse_coord_gloss_logits"):
        lp = torch.log_softmax(out[k].detach().permute(1, 0, 2), -1).clamp(-100, 0)
        nll = model.loss_fn(lp, src["gloss_labels"].int(), torch.maximum(src["valid_len_in"], src["gloss_lengths"]).int(),
                            src["gloss_lengths"].int())
        assert bool(torch.isfinite(nll).all()), nll
        per_sample[k] = [float(x) for x in nll]

    l32, n32 = train(model_from(state, cfg, vocab), src, torch.float32)
    l64, n64 = train(model_from(state, cfg, vocab), src, torch.float64)
    assert (n32 > CLIP).all(), n32  # the clip is active at every step
    floor = float(max(np.abs(l32 - l64).max() / np.abs(l64).max(), np.abs(n32 - n64).max() / np.abs(n64).max()))
    arrs.update({"train.total_loss": l32, "train.grad_norm": n32, "train.total_loss_fp64": l64,
                 "train.grad_norm_fp64": n64})

    nfiles = save_parts("model_small", arrs)
    assert nfiles <= 4, nfiles
    nparams = sum(v.numel() for v in state.values())
    manifest = {"torch": torch.__version__, "reference": "tinh2044/SCAttenNet @ 2025-07-18", "fixtures": {
        "model_small": {"op": "MSCA_Net (eval) forward + backward of total_loss", "ref": "model/__init__.py:72-290",
                        "cfg": cfg, "vocab": vocab, "B": 3, "T": 26, "K_all": 16, "files": nfiles, "params": nparams,
                        "no_grad": no_grad, "losses": losses, "max_abs_logit": max_logit,
                        "per_sample_ctc": per_sample,
                        "conditions": {"losses_below_clamp": True, "logits_inside_50": True,
                                       "per_sample_ctc_finite": True}},
        "model_train_steps": {"op": "opt.py:28-38 x 6, model in eval() (dropout off: stated deviation)",
                              "arrays": "train.* in model_small*.npz", "steps": STEPS, "adam": ADAM, "clip": CLIP,
                              "total_loss": l32.tolist(), "grad_norm": n32.tolist(), "clip_active_every_step": True,
                              "fp64_vs_fp32_rel": floor}}}
    with open(os.path.join(HERE, "manifest_model.json"), "w") as f:
        json.dump(manifest, f, indent=1)
    print("wrote", nfiles, "files;", nparams, "parameters; losses", losses, "train", l32, "floor", floor)


def model_from(state, cfg, vocab):
    m = MSCA_Net(copy.deepcopy(cfg), list(range(vocab)), device="cpu")
    m.load_state_dict(state)
    return m


if __name__ == "__main__":
    main()
