"""Time ensemble distillation (scattennet_amd/distill.py, sca_distill_heads_fwd / _bwd) on one
MI355X at the training shape of the 2014T yaml: B = 8 clips, T/4 = 64 logit frames, C = 1124, for
(G members, S students) = (1, 4), (3, 3) and (5, 3), in both modes, forward + backward, against
the composition it replaces:

  for every student s: distillation_loss(students[s], ensemble_log_probs(members, ...), w_s)

(one ensemble launch, then a row kernel, a finalize and a gradient kernel per student: 1 + 3 S
launches against 3; with G = 1 the composition is `distillation_loss` on the member itself, 3 S
launches).  All are captured graphs of --calls calls each (device time of the launches only),
timed with device events around --replays replays per window, in alternated windows; us per call
as median and range over --windows windows (the method of tools/ensemble_bench.py).  Losses and
student gradients of the two forms are compared (maximum absolute difference) before anything is
timed.  Every variant owns its leaves.  Synthetic logits N(0, 3^2).  Needs a GPU.

--learned: the weights are softmax(theta) with theta on the device, in both forms.
--forms composed: the composition alone, which an older build of the library (SCA_LIB_PATH) runs too:
the yardstick at the parent commit.

Usage: python tools/distill_bench.py [--B 8] [--T 64] [--C 1124] [--cases 1,4 3,3 5,3] [--calls 100]
                                     [--replays 5] [--windows 7] [--learned] [--forms grouped composed]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.align_bench import alternated, graph_of  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--cases", nargs="+", default=["1,4", "3,3", "5,3"], help="G,S pairs")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--learned", action="store_true", help="weights from theta on the device, in both forms")
    ap.add_argument("--forms", nargs="+", default=["grouped", "composed"], choices=["grouped", "composed"],
                    help="composed alone also runs on a library without the grouped entries (SCA_LIB_PATH)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distill_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    from scattennet_amd.ensemble import MODES
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    out = {"workload": "ensemble distillation forward + backward: the grouped call against distillation_loss per "
                       "student on ensemble_log_probs; captured graphs, device events",
           "B": a.B, "T": a.T, "C": a.C, "learned": a.learned, "forms": a.forms, "calls_per_graph": a.calls,
           "replays_per_window": a.replays, "windows": a.windows, "unit": "us per call", "cases": []}
    for pair in a.cases:
        G, Sn = (int(v) for v in pair.split(","))
        xs = [(torch.randn(a.B, a.T, a.C, generator=gen) * 3).to(dev) for _ in range(G)]
        ss = [(torch.randn(a.B, a.T, a.C, generator=gen) * 3).to(dev) for _ in range(Sn)]
        sw = [1.0 / (1 + s) for s in range(Sn)]
        theta = torch.linspace(-0.5, 0.5, G).to(dev)
        kw = {"weight_logits": theta} if a.learned else {"weights": None}
        dl = torch.ones(Sn, device=dev)
        dls = list(dl.unbind(0))  # the composition's incoming gradients: views, no launch of their own

        def leaves():
            return [x.detach().clone().requires_grad_(True) for x in ss]

        def fwd_bwd(form, mode, zs):
            def fn():
                for z in zs:
                    z.grad = None
                if form == "grouped":
                    losses = S.ensemble_distillation_loss(zs, xs, sw, mode=mode, **kw)
                    losses.backward(dl)
                    return [losses.detach()] + [z.grad for z in zs]
                e = xs[0] if G == 1 else S.ensemble_log_probs(xs, mode=mode, **kw)
                losses = [S.distillation_loss(z, e, w) for z, w in zip(zs, sw)]
                torch.autograd.backward(losses, dls)  # nothing but the project's own launches is timed
                return [[x.detach() for x in losses]] + [z.grad for z in zs]
            return fn

        graphs, diff = {}, {}
        for mode in MODES:
            if len(a.forms) == 2:
                side = torch.cuda.Stream()  # the comparison, on leaves of its own and off the default stream
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    gf, gt = fwd_bwd("grouped", mode, leaves())(), fwd_bwd("composed", mode, leaves())()
                    gt[0] = torch.stack(gt[0])
                    diff[mode] = {"losses": float((gf[0] - gt[0]).abs().max()), "loss_max": float(gt[0].abs().max()),
                                  "gradients": max(float((p - q).abs().max()) for p, q in zip(gf[1:], gt[1:])),
                                  "gradient_max": max(float(q.abs().max()) for q in gt[1:])}
                torch.cuda.current_stream().wait_stream(side)
            for form in a.forms:
                graphs[f"{form}_{mode}"] = graph_of(fwd_bwd(form, mode, leaves()), a.calls)
        for gr, _ in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        case = {"G": G, "S": Sn, "launches_grouped": 3, "launches_composed": (1 if G > 1 else 0) + 3 * Sn,
                "max_abs_diff_grouped_vs_composed": diff}
        case.update(alternated(graphs, a.calls, a.replays, a.windows))
        for mode in MODES if len(a.forms) == 2 else ():
            f, t = case[f"grouped_{mode}"], case[f"composed_{mode}"]
            case[f"composed_over_grouped_{mode}"] = round(t["median"] / f["median"], 2)
            case[f"grouped_below_composed_range_{mode}"] = f["median"] < t["min"]
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
