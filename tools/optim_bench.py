"""Time the fused clip + Adam update against the reference's own calls (not part of bench.py).

On a workload's parameter set (default cfg2: 4 SCA streams, 25.84 M parameters) with random
gradients present, after warm-up, in one process:

* fused — a hipGraph holding only FusedAdam.step() (two launches), `--steps` replays;
* stock — `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam.step()` (opt.py:34-35),
  eagerly, `--steps` times, on clones of the same tensors.

The two are alternated `--rounds` times; each round is timed with device events around the
whole window (ending in a synchronise).  Bytes: 32 per parameter (pass 1 reads g; pass 2
reads p, g, m, v and writes p, m, v).  Prints one JSON line; `--chunk` / `--max-blocks` take
several values to compare grid shapes in the same run.

  python tools/optim_bench.py [--workload cfg2] [--steps 50] [--rounds 5] [--chunk 8192 ...]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes / s
YAML = dict(lr=0.002, betas=(0.9, 0.998), eps=1e-8, weight_decay=2e-5)  # configs/phoenix-2014t.yaml:195-206


def timed(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk", type=int, nargs="+", default=None)
    ap.add_argument("--max-blocks", type=int, nargs="+", default=[0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench needs a GPU")
    from scattennet_amd import FusedAdam, optim, workloads as W
    dev = torch.device("cuda:0")
    model = W.build_streams(W.WORKLOADS[args.workload], dev, seed=0, init="random")
    params = [p for p in model.parameters()]
    gen = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-2
    n = sum(p.numel() for p in params)
    nbytes = 32 * n

    runs = {}
    for chunk in (args.chunk or [optim.CHUNK]):
        for mb in args.max_blocks:
            opt = FusedAdam(params, max_grad_norm=1.0, chunk=chunk, max_blocks=mb, **YAML)
            for _ in range(args.warmup):
                opt.step()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
            graph.replay()
            runs[(chunk, mb)] = (opt, graph)

    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for c, p in zip(clones, params):
        c.grad = p.grad.clone()
    stock = torch.optim.Adam(clones, **YAML)

    def stock_step():
        torch.nn.utils.clip_grad_norm_(clones, max_norm=1.0)
        stock.step()

    for _ in range(args.warmup):
        stock_step()
    times = {k: [] for k in list(runs) + ["stock"]}
    for _ in range(args.rounds):
        for k, (_, graph) in runs.items():
            times[k].append(timed(graph.replay, args.steps))
        times["stock"].append(timed(stock_step, args.steps))

    def report(ts):
        ms = statistics.median(ts)
        return {"ms": round(ms, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                "GBps": round(nbytes / ms / 1e6, 1), "hbm_peak_frac": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}

    best = min(runs, key=lambda k: statistics.median(times[k]))
    out = {"tool": "optim_bench", "workload": args.workload, "tensors": len(params), "parameters": n,
           "bytes_per_step": nbytes, "steps": args.steps, "rounds": args.rounds,
           "fused": {f"chunk{c}_blocks{b}": report(times[(c, b)]) for c, b in runs},
           "stock_clip_plus_adam": report(times["stock"]),
           "fused_best": f"chunk{best[0]}_blocks{best[1]}",
           "speedup_vs_stock": round(statistics.median(times["stock"]) / statistics.median(times[best]), 2),
           "grad_norm": float(runs[best][0].grad_norm), "steps_applied": int(runs[best][0].step_count)}
    print(json.dumps(out))
    if statistics.median(times[best]) > statistics.median(times["stock"]):
        raise SystemExit("fused step slower than the stock calls")


if __name__ == "__main__":
    main()
