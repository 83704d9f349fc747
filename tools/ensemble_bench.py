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

--backward times forward + backward instead: `ensemble_log_probs(..., differentiable=True)` and one
launch of `sca_ensemble_log_probs_bwd` for all members, against autograd through the same torch
composition, under one fixed incoming gradient N(0, 1); every variant owns its leaves.  The members'
gradients of the two forms are compared (maximum absolute difference) before anything is timed, on
leaves of their own.  The bytes are the forward's plus the backward's: "prob" reads the G members,
out and dout and writes G gradients, "logprob" reads out and dout and writes G gradients.

--learned times the learned ensemble (`ensemble_log_probs(weight_logits=theta)`,
sca_ensemble_log_probs_dw): the forward against the host-weight call with the same weights in the
same run (is the median inside that call's own window-to-window range?), and with --backward
forward + backward with d theta against the same call without it (the price of the weight
gradient: the partial stores and the summing launch, in "logprob" also the member reads) and
against autograd through the torch composition with theta a leaf.  Outputs and gradients of the
forms are compared before anything is timed.

Usage: python tools/ensemble_bench.py [--B 8] [--T 64] [--C 1124] [--members 2 5] [--calls 100]
                                      [--replays 5] [--windows 7] [--backward] [--learned]
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


def learned_composition(xs, theta, mode):
    lw = torch.log_softmax(theta, 0)
    lps = [torch.log_softmax(x, -1) for x in xs]
    if mode == "prob":
        return torch.logsumexp(torch.stack([lp + lw[g] for g, lp in enumerate(lps)]), 0)
    u = torch.exp(lw[0]) * lps[0]
    for g in range(1, len(lps)):
        u = u + torch.exp(lw[g]) * lps[g]
    return torch.log_softmax(u, -1)


def learned_case(a, S, modes, G, xs, dout, dev):
    """One G of --learned: the graphs' times and the comparisons made before timing."""
    theta0 = torch.linspace(-0.5, 0.5, G)
    weights = torch.softmax(theta0.double(), 0).tolist()
    theta = theta0.to(dev)
    graphs, diff = {}, {}

    def leaves(with_theta):
        return [x.detach().clone().requires_grad_(True) for x in xs], theta.clone().requires_grad_(with_theta)

    def fwd_bwd(form, mode, zs, th):
        def fn():
            for z in zs + [th]:
                z.grad = None
            y = learned_composition(zs, th, mode) if form == "torch" else \
                S.ensemble_log_probs(zs, None, mode, weight_logits=th, differentiable=True)
            y.backward(dout)
            return [z.grad for z in zs] + [th.grad]
        return fn

    for mode in modes:
        if a.backward:
            side = torch.cuda.Stream()  # the comparison, on leaves of its own and off the default stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                gf, gt = fwd_bwd("fused", mode, *leaves(True))(), fwd_bwd("torch", mode, *leaves(True))()
                diff[mode] = {"members": max(float((p - q).abs().max()) for p, q in zip(gf[:-1], gt[:-1])),
                              "dtheta": float((gf[-1] - gt[-1]).abs().max()), "dtheta_max": float(gt[-1].abs().max())}
            torch.cuda.current_stream().wait_stream(side)
            graphs[f"learned_dtheta_{mode}"] = graph_of(fwd_bwd("fused", mode, *leaves(True)), a.calls)
            graphs[f"learned_members_{mode}"] = graph_of(fwd_bwd("fused", mode, *leaves(False)), a.calls)
            graphs[f"torch_{mode}"] = graph_of(fwd_bwd("torch", mode, *leaves(True)), a.calls)
        else:
            host = lambda mode=mode: S.ensemble_log_probs(xs, weights, mode)  # noqa: E731
            learned = lambda mode=mode: S.ensemble_log_probs(xs, None, mode, weight_logits=theta)  # noqa: E731
            diff[mode] = float((host() - learned()).abs().max())
            graphs[f"host_{mode}"] = graph_of(host, a.calls)
            graphs[f"learned_{mode}"] = graph_of(learned, a.calls)
    for gr, _ in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    case = {"G": G, "max_abs_diff": diff}
    case.update(alternated(graphs, a.calls, a.replays, a.windows))
    for mode in modes:
        if a.backward:
            d, m, t = (case[f"{k}_{mode}"] for k in ("learned_dtheta", "learned_members", "torch"))
            case[f"dtheta_price_us_{mode}"] = round(d["median"] - m["median"], 2)
            case[f"torch_over_learned_{mode}"] = round(t["median"] / d["median"], 2)
            case[f"learned_below_torch_range_{mode}"] = d["median"] < t["min"]
        else:
            h, le = case[f"host_{mode}"], case[f"learned_{mode}"]
            case[f"learned_over_host_{mode}"] = round(le["median"] / h["median"], 3)
            case[f"learned_inside_host_range_{mode}"] = h["min"] <= le["median"] <= h["max"]
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--members", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--backward", action="store_true", help="time forward + backward of the differentiable call "
                                                             "against autograd through the torch composition")
    ap.add_argument("--learned", action="store_true", help="time the learned ensemble (weight_logits on the device) "
                                                            "against the host-weight call, with --backward the "
                                                            "price of d theta and autograd through the composition")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    from scattennet_amd.ensemble import MODES
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    what = "ensemble_log_probs forward + backward against autograd through" if a.backward else "ensemble_log_probs against"
    out = {"workload": what + " the torch composition it replaces; captured graphs, device events",
           "B": a.B, "T": a.T, "C": a.C, "calls_per_graph": a.calls, "replays_per_window": a.replays,
           "windows": a.windows, "unit": "us per call", "cases": []}
    if a.learned:
        out["workload"] = ("learned ensemble forward + backward: with d theta, without it, autograd through the torch "
                           "composition with theta a leaf" if a.backward else
                           "learned ensemble forward against the host-weight call") + "; captured graphs, device events"
    for G in a.members:
        xs = [(torch.randn(a.B, a.T, a.C, generator=gen) * 3).to(dev) for _ in range(G)]
        if a.learned:
            dout = torch.randn(a.B, a.T, a.C, generator=gen).to(dev)
            out["cases"].append(learned_case(a, S, MODES, G, xs, dout, dev))
            continue
        weights = [1.0 / G] * G
        graphs, diff = {}, {}
        dout = torch.randn(a.B, a.T, a.C, generator=gen).to(dev)

        def leaves():
            return [x.detach().clone().requires_grad_(True) for x in xs]

        def fwd_bwd(form, mode, zs):
            def fn():
                for z in zs:
                    z.grad = None
                y = S.ensemble_log_probs(zs, None, mode, differentiable=True) if form == "fused" else \
                    torch_composition(zs, weights, mode)
                y.backward(dout)
                return [z.grad for z in zs]
            return fn

        for mode in MODES if a.backward else ():
            side = torch.cuda.Stream()  # the comparison, on leaves of its own and off the default stream
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                gf, gt = fwd_bwd("fused", mode, leaves())(), fwd_bwd("torch", mode, leaves())()
                diff[mode] = max(float((p - q).abs().max()) for p, q in zip(gf, gt))
            torch.cuda.current_stream().wait_stream(side)
            graphs[f"fused_{mode}"] = graph_of(fwd_bwd("fused", mode, leaves()), a.calls)
            graphs[f"torch_{mode}"] = graph_of(fwd_bwd("torch", mode, leaves()), a.calls)
        for mode in () if a.backward else MODES:
            fused = lambda mode=mode: S.ensemble_log_probs(xs, None, mode)  # noqa: E731
            composed = lambda mode=mode: torch_composition(xs, weights, mode)  # noqa: E731
            diff[mode] = float((fused() - composed()).abs().max())
            graphs[f"fused_{mode}"] = graph_of(fused, a.calls)
            graphs[f"torch_{mode}"] = graph_of(composed, a.calls)
        for gr, _ in graphs.values():
            gr.replay()
        torch.cuda.synchronize()
        row = a.B * a.T * a.C * 4
        nbytes = {mode: (G + 1) * row for mode in MODES}
        if a.backward:
            nbytes = {"prob": (G + 1 + 2 * G + 2) * row, "logprob": (G + 1 + G + 2) * row}
        case = {"G": G, "bytes_moved_at_least": nbytes if a.backward else (G + 1) * row,
                "max_abs_diff_fused_vs_torch": diff}
        case.update(alternated(graphs, a.calls, a.replays, a.windows))
        for mode in MODES:
            f, t = case[f"fused_{mode}"], case[f"torch_{mode}"]
            case[f"torch_over_fused_{mode}"] = round(t["median"] / f["median"], 2)
            case[f"fused_below_torch_range_{mode}"] = f["median"] < t["min"]
            case[f"fused_GBps_{mode}"] = round(nbytes[mode] / (f["median"] * 1e-6) / 1e9, 1)
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
