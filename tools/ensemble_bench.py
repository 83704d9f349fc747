"""Time the head ensemble (scattennet_amd/ensemble.py, sca_ensemble_log_probs) on one MI355X at
the evaluation shape of the 2014T yaml: B = 8 clips, T/4 = 64 logit frames, C = 1124, for G = 2
and G = 5 members, in both modes, against the torch composition it replaces:

  "prob":    torch.logsumexp(torch.stack([log_softmax(x_g) + log w_g]), 0)
  "logprob": log_softmax(sum_g w_g log_softmax(x_g))

All are captured graphs of --calls calls each (device time of the launches only), timed with
device events around --replays replays per window, in alternated windows; us per call as median
and range over --windows windows.  From the shapes: the bytes the fused call must move (G reads
and one write of (B, T, C) fp32) and the rate that gives.  The outputs of the two forms are
compared (maximum absolute difference) before anything is timed.  Synthetic logits N(0, 3^2).
Needs a GPU.

Usage: python tools/ensemble_bench.py [--B 8] [--T 64] [--C 1124] [--members 2 5] [--calls 100]
                                      [--replays 5] [--windows 7]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.align_bench import alternated, graph_of  # noqa: E402


def torch_composition(xs, weights, mode):
    if mode == "prob":
        return torch.logsumexp(torch.stack([torch.log_softmax(x, -1) + math.log(w) for x, w in zip(xs, weights)]), 0)
    u = weights[0] * torch.log_softmax(xs[0], -1)
    for x, w in zip(xs[1:], weights[1:]):
        u = u + w * torch.log_softmax(x, -1)
    return torch.log_softmax(u, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--members", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    from scattennet_amd.ensemble import MODES
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    out = {"workload": "ensemble_log_probs against the torch composition it replaces; captured graphs, device events",
           "B": a.B, "T": a.T, "C": a.C, "calls_per_graph": a.calls, "replays_per_window": a.replays,
           "windows": a.windows, "unit": "us per call", "cases": []}
    for G in a.members:
        xs = [(torch.randn(a.B, a.T, a.C, generator=gen) * 3).to(dev) for _ in range(G)]
        weights = [1.0 / G] * G
        graphs, diff = {}, {}
        for mode in MODES:
            fused = lambda mode=mode: S.ensemble_log_probs(xs, None, mode)  # noqa: E731
            composed = lambda mode=mode: torch_composition(xs, weights, mode)  # noqa: E731
            diff[mode] = float((fused() - composed()).abs().max())
            graphs[f"fused_{mode}"] = graph_of(fused, a.calls)
            graphs[f"torch_{mode}"] = graph_of(composed, a.calls)
        for gr, _ in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        nbytes = (G + 1) * a.B * a.T * a.C * 4
        case = {"G": G, "bytes_moved_at_least": nbytes, "max_abs_diff_fused_vs_torch": diff}
        case.update(alternated(graphs, a.calls, a.replays, a.windows))
        for mode in MODES:
            f, t = case[f"fused_{mode}"], case[f"torch_{mode}"]
            case[f"torch_over_fused_{mode}"] = round(t["median"] / f["median"], 2)
            case[f"fused_below_torch_range_{mode}"] = f["median"] < t["min"]
            case[f"fused_GBps_{mode}"] = round(nbytes / (f["median"] * 1e-6) / 1e9, 1)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
