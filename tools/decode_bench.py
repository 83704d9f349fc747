"""Time the evaluation ops (scattennet_amd/decode.py) on one MI355X: greedy CTC decoding,
prefix beam search and the WER counts, at the evaluation shape of the 2014T yaml (B = 8,
T/4 = 64, C = 1124, beam 5 as main.py sets it).  Each op is timed two ways: eager calls
(Python, allocator and launch overhead included) and replays of a captured graph (device time
of the launches only).  Both windows end in a device synchronise; the figure is the median
of --repeats windows of --steps calls, with the spread (min, max) beside it.  Synthetic
logits N(0, 4^2), full-length clips (the longest dependent chain).  Needs a GPU.

Usage: python tools/decode_bench.py [--B 8] [--T 64] [--C 1124] [--beam 5] [--steps 200]

--heads G: the G heads of one forward (G different logit tensors, 1 <= G <= 8) decoded by one
grouped call (ctc_decode_heads_device) against G sequential single-head calls of the same build.
Both are captured graphs, timed in alternated windows of --steps replays, each window ending in
a device synchronise; median (min, max) over --repeats windows, and whether the grouped median
lies below the whole range of the sequential windows.  The eager forms are timed the same way.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def windows(fn, steps, repeats):
    """us per call: (median, min, max) over `repeats` windows of `steps` calls."""
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / steps)
    return [round(v, 1) for v in (statistics.median(out), min(out), max(out))]


def graphed(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def alternated(fns, steps, repeats):
    """us per call per variant, [median, min, max] and the windows, the variants taking turns."""
    out = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e6 / steps)
    return {k: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                "windows": [round(x, 1) for x in v]} for k, v in out.items()}


def heads_mode(a, S, dev):
    g = torch.Generator().manual_seed(0)
    xs = [(torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev) for _ in range(a.heads)]
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    grouped = lambda: S.ctc_decode_heads_device(xs, il, a.beam)  # noqa: E731
    sequential = lambda: [S.ctc_decode_device(x, il, a.beam) for x in xs]  # noqa: E731
    got, want = grouped(), sequential()
    for h in range(a.heads):  # the two variants compute the same thing
        assert all(torch.equal(got[i][h], want[h][i]) for i in range(3)), h
    res = {"workload": "CTC beam decode of G heads: one grouped call against G single-head calls", "heads": a.heads,
           "B": a.B, "T": a.T, "C": a.C, "beam": a.beam, "steps": a.steps, "repeats": a.repeats, "unit": "us per call"}
    eager = {"grouped": grouped, "sequential": sequential}
    for fn in eager.values():
        for _ in range(a.warmup):
            fn()
    res["eager"] = alternated(eager, a.steps, a.repeats)
    graphs = {k: graphed(fn) for k, fn in eager.items()}
    for fn in graphs.values():
        for _ in range(a.warmup):
            fn()
    res["graph"] = alternated(graphs, a.steps, a.repeats)
    for k in ("eager", "graph"):
        res[k]["grouped_median_below_sequential_range"] = res[k]["grouped"]["median"] < res[k]["sequential"]["min"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--S", type=int, default=24, help="reference length for the WER counts")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--heads", type=int, default=0, help="G > 0: one grouped call against G single-head calls")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    dev = torch.device("cuda")
    if a.heads:
        return heads_mode(a, S, dev)
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(a.B, a.T, a.C, generator=g) * 4).to(dev)
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    ref = torch.randint(1, a.C, (a.B, a.S), generator=g).to(device=dev, dtype=torch.int32)
    ref_len = torch.full((a.B,), a.S, dtype=torch.int32, device=dev)
    tokens, lengths, _ = S.ctc_decode_device(x, il, a.beam)
    ops = {
        "greedy": lambda: S.ctc_greedy_decode_device(x, il),
        f"beam{a.beam}": lambda: S.ctc_decode_device(x, il, a.beam),
        "wer_counts": lambda: S.wer_counts(ref, ref_len, tokens, lengths),
        f"beam{a.beam}+wer": lambda: S.wer_counts(ref, ref_len, *S.ctc_decode_device(x, il, a.beam)[:2]),
    }
    res = {"workload": "CTC decode + WER counts", "B": a.B, "T": a.T, "C": a.C, "beam": a.beam, "S": a.S,
           "steps": a.steps, "repeats": a.repeats, "unit": "us per call: [median, min, max]"}
    for name, fn in ops.items():
        for _ in range(a.warmup):
            fn()
        res[name + "_eager"] = windows(fn, a.steps, a.repeats)
        replay = graphed(fn)
        for _ in range(a.warmup):
            replay()
        res[name + "_graph"] = windows(replay, a.steps, a.repeats)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
