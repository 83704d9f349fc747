"""Time the evaluation ops (scattennet_amd/decode.py) on one MI355X: greedy CTC decoding,
prefix beam search and the WER counts, at the evaluation shape of the 2014T yaml (B = 8,
T/4 = 64, C = 1124, beam 5 as main.py sets it).  Each op is timed two ways: eager calls
(Python, allocator and launch overhead included) and replays of a captured graph (device time
of the launches only).  Both windows end in a device synchronise; the figure is the median
of --repeats windows of --steps calls, with the spread (min, max) beside it.  Synthetic
logits N(0, 4^2), full-length clips (the longest dependent chain).  Needs a GPU.

Usage: python tools/decode_bench.py [--B 8] [--T 64] [--C 1124] [--beam 5] [--steps 200]
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    dev = torch.device("cuda")
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
