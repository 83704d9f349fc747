"""Golden vectors for the training update (scattennet_amd/optim.py), from the REFERENCE.

Runs ONLY in the build container, where `/root/reference` is importable: the reference's
optimizer.py (build_optimizer, WarmupCosineAnnealingScheduler) is imported and driven with the
`training.optimization` section of configs/phoenix-2014t.yaml.  Writes numeric arrays only:

* optim_schedule.npz — the learning rates of the reference scheduler over its 100 epochs
  (one column per parameter group);
* optim_adam_steps.npz (+ .partN.npz) — six steps of opt.py:34-35, clip_grad_norm_(..., 1.0) then
  optimizer.step(), on a toy module with two children (one matched by a substring lr
  override, one on the default rate): initial parameters, every step's gradients (scaled
  x10 and x1e-3 in turn, so the clip is active on steps 1, 3, 5 and idle on 2, 4, 6), the norms
  clip_grad_norm_ returned, and parameters and moments after steps 1, 3 and 6;
* manifest_optim.json — torch version, seed, hyper-parameters and the parameter layout.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_optim.py
"""
import copy
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import optimizer as ref_optim  # noqa: E402
from tests.golden_util import save_parts  # noqa: E402

SEED = 20250718
OVERRIDE = {"mapping": 0.0005}  # substring of the first child's name
LAYOUT = {"coord_mapping": [(1,), (5,), (4097,), (258, 64)], "body_stream": [(3,), (257,), (8199,)]}
SCALES = [10.0, 1e-3, 10.0, 1e-3, 10.0, 1e-3]
SAVE_AFTER = (1, 3, 6)


class Bag(torch.nn.Module):
    def __init__(self, shapes, gen):
        super().__init__()
        self.items = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes])


def toy(gen):
    m = torch.nn.Module()
    for name, shapes in LAYOUT.items():
        m.add_module(name, Bag(shapes, gen))
    return m


def section():
    cfg = yaml.safe_load(open(os.path.join(REF, "configs", "phoenix-2014t.yaml")))
    return cfg["training"]["optimization"]


def main():
    torch.manual_seed(SEED)
    gen = torch.Generator().manual_seed(SEED)
    opt_cfg = section()
    cfg = copy.deepcopy(opt_cfg)
    cfg["learning_rate"].update(OVERRIDE)

    # the schedule
    model = toy(gen)
    opt = ref_optim.build_optimizer(copy.deepcopy(cfg), model)
    sched, unit = ref_optim.build_scheduler(copy.deepcopy(cfg), opt)
    assert unit == "epoch"
    rates = []
    for _ in range(int(cfg["total_epochs"])):
        rates.append([g["lr"] for g in opt.param_groups])
        opt.step()
        sched.step()
    np.savez(os.path.join(HERE, "optim_schedule.npz"), lr=np.array(rates, dtype=np.float64))

    # six clipped Adam steps
    model = toy(gen)
    opt = ref_optim.build_optimizer(copy.deepcopy(cfg), model)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    arrs = {f"init.{n}": p.detach().numpy().copy() for n, p in zip(names, params)}
    norms = []
    for step, scale in enumerate(SCALES, start=1):
        for n, p in zip(names, params):
            p.grad = torch.randn(p.shape, generator=gen) * scale
            arrs[f"grad{step}.{n}"] = p.grad.numpy().copy()
        norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)))
        opt.step()
        if step in SAVE_AFTER:
            for n, p in zip(names, params):
                st = opt.state[p]
                assert int(st["step"]) == step
                arrs[f"p{step}.{n}"] = p.detach().numpy().copy()
                arrs[f"exp_avg{step}.{n}"] = st["exp_avg"].numpy().copy()
                arrs[f"exp_avg_sq{step}.{n}"] = st["exp_avg_sq"].numpy().copy()
    arrs["norms"] = np.array(norms, dtype=np.float64)
    parts = save_parts("optim_adam_steps", arrs, HERE)

    g0 = opt.param_groups[0]
    manifest = {
        "torch": torch.__version__, "reference": "tinh2044/SCAttenNet @ 2025-07-18", "seed": SEED,
        "source": "reference optimizer.py build_optimizer / build_scheduler, imported; "
                  "configs/phoenix-2014t.yaml training.optimization",
        "config": opt_cfg, "lr_override": OVERRIDE, "max_norm": 1.0, "scales": SCALES,
        "save_after": list(SAVE_AFTER), "parts": parts,
        "layout": {k: [list(s) for s in v] for k, v in LAYOUT.items()}, "names": names,
        "groups": [{"lr": g["lr"], "betas": list(g["betas"]), "eps": g["eps"], "weight_decay": g["weight_decay"],
                    "amsgrad": g["amsgrad"], "params": len(g["params"])} for g in opt.param_groups],
        "optimizer": type(opt).__name__, "group_keys": sorted(k for k in g0 if k != "params"),
    }
    json.dump(manifest, open(os.path.join(HERE, "manifest_optim.json"), "w"), indent=1)
    print("norms", norms, "parts", parts)


if __name__ == "__main__":
    main()
