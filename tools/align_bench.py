"""Time CTC forced alignment (scattennet_amd/align.py, sca_ctc_align_heads) on one MI355X at the
evaluation shape of the 2014T yaml: G = 2 heads, B = 8 clips, T/4 = 64 logit frames, C = 1124,
each head aligned to its own hypotheses from the beam decode (beam 5) of the same logits, as
eval_step does with align=True.  From the same run it times the grouped beam decode of the same
heads, the figure the alignment is to be read against, and the alignment of the same heads to
shared references of --references (24) random labels per clip (49 extended states: the path
that needs no barrier).

Both are captured graphs of --calls calls each (device time of the launches only), timed with
device events around --replays replays per window, in alternated windows; us per call as median
and range over --windows windows.  Synthetic logits N(0, 4^2), full-length clips (the longest
dependent chain); --blank-bias b adds b to the blank logit of a random 70 % of the frames, which
gives hypotheses of a realistic length instead of one label per frame.  Needs a GPU.

Usage: python tools/align_bench.py [--heads 2] [--B 8] [--T 64] [--C 1124] [--beam 5]
                                   [--blank-bias 0] [--references 24] [--calls 100] [--replays 5] [--windows 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def graph_of(fn, calls):
    """One captured graph of `calls` calls of fn (warmed up on a side stream, as capture needs)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(calls)]
    return g, keep


def alternated(graphs, calls, replays, windows):
    """us per call per variant: median, min, max and the windows, the variants taking turns."""
    out = {k: [] for k in graphs}
    for _ in range(windows):
        for k, (g, _) in graphs.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(replays):
                g.replay()
            end.record()
            torch.cuda.synchronize()
            out[k].append(start.elapsed_time(end) * 1e3 / (calls * replays))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                "windows": [round(x, 2) for x in v]} for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--blank-bias", type=float, default=0.0)
    ap.add_argument("--references", type=int, default=24, help="also align to shared references of this many labels "
                                                               "(0: skip)")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--replays", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("align_bench: needs a GPU; nothing is measured without one")
    import scattennet_amd as S
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    xs = []
    for _ in range(a.heads):
        x = torch.randn(a.B, a.T, a.C, generator=g) * 4
        if a.blank_bias:
            x[:, :, 0] += a.blank_bias * (torch.rand(a.B, a.T, generator=g) < 0.7)
        xs.append(x.to(dev))
    il = torch.full((a.B,), a.T, dtype=torch.int32, device=dev)
    tokens, lengths, _ = S.ctc_decode_heads_device(xs, il, a.beam)
    decode = lambda: S.ctc_decode_heads_device(xs, il, a.beam)  # noqa: E731
    align = lambda: S.ctc_align_heads_device(xs, il, tokens, lengths)  # noqa: E731
    res = align()
    assert bool(torch.isfinite(res.scores).all())  # a hypothesis can always be emitted by its own logits
    graphs = {"align": graph_of(align, a.calls), "beam_decode": graph_of(decode, a.calls)}
    if a.references:  # shared references of --references labels per clip: L <= 64 is the barrier-free path
        ref = torch.randint(1, a.C, (a.B, a.references), generator=g).to(device=dev, dtype=torch.int32)
        ref_len = torch.full((a.B,), a.references, dtype=torch.int32, device=dev)
        graphs["align_references"] = graph_of(lambda: S.ctc_align_heads_device(xs, il, ref, ref_len), a.calls)
    for gr, _ in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    out = {"workload": "CTC forced alignment of G heads to their own beam hypotheses, against the grouped beam "
                       "decode of the same heads; captured graphs, device events", "heads": a.heads, "B": a.B,
           "T": a.T, "C": a.C, "S": a.T, "beam": a.beam, "blank_bias": a.blank_bias, "references": a.references,
           "hypothesis_length": {"mean": round(float(lengths.float().mean()), 1), "min": int(lengths.min()),
                                 "max": int(lengths.max())},
           "calls_per_graph": a.calls, "replays_per_window": a.replays, "windows": a.windows, "unit": "us per call"}
    out.update(alternated(graphs, a.calls, a.replays, a.windows))
    out["align_over_decode"] = round(out["align"]["median"] / out["beam_decode"]["median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
