"""Time the whole MSCA_Net training step (scattennet_amd.train_step: forward, finite guard,
backward of total_loss, FusedAdam) on one MI355X at the Phoenix-2014T yaml shapes: B = 8,
T = 256, BASELINE config 3's encoder, heads with vocabulary C (1124), BiLSTM alignment head
(1024 -> 2 x 512, 2 layers), 24 glosses per clip.  Synthetic data, eval mode (dropout off),
as tools/heads_bench.py.

Three variants of the same step:
  graph_off    one captured hipGraph, model.check = "off"   (no scan; the report launch stays)
  graph_defer  one captured hipGraph, model.check = "defer" (scan + report, no host read)
  eager_sync   eager launches + read_report() every step     (one host read per step)
The two graphs are timed in alternated windows (device events around `--steps` replays each)
and reported as medians over `--windows` windows; the scan's cost is defer - off.  The scan
kernel alone is timed as a captured graph of `--scan-reps` sca_finite_scan calls over
tensors of the step's shapes (they stay cache-resident between calls: the figure is the
kernel's rate on 25.6 MB it re-reads, not an HBM stream).  Prints one JSON line.

Usage: python tools/model_bench.py [--B 8] [--T 256] [--C 1124] [--steps 10] [--windows 7]

--mixed: a stream of batches whose length varies, as a training collator produces it.  A fixed
seeded sequence of `--batches` (20) batches of B clips; every clip's length is drawn with
select_frames' training rule (a target in [0.5 n, 1.5 n] capped at max_len = T) from a source
length n ~ U[40, 240], the batch is padded to its longest clip.  Two ways to train on it:
  eager      train_step per batch at the batch's own T        (what a varying T costs today)
  bucketed   BucketedTrainStep, buckets --buckets (64,128,192,256), every graph captured before
Both are timed over whole passes of the stream (host clock around the pass, ending in a device
synchronise; no report read in either) in alternated windows; ms/step as median and range over
`--windows`.  Then, per bucket, the padding overhead: the bucket's replay with a batch just
above the previous bucket against a hipGraph captured at exactly that T (alternated windows of
`--steps` steps).  `--eager-only` times the eager pass alone and `--root DIR` imports the
package from another checkout (the same eager measurement on an earlier commit).  One JSON line.

--eval (with --mixed): an evaluation pass over the same stream, beam --beam (5), two ways:
  loop       what a user can write without the evaluation step: per batch a no-grad eager forward
             (check "defer"), decode_outputs' two halves per "gloss_logits" head (ctc_decode_device,
             then one packed device-to-host copy of tokens, lengths and total_loss: the batch's one
             host read) with wer_counts on the device between them
  bucketed   BucketedEvalStep (buckets --buckets, every graph captured before), read() at the end
Whole passes on the host clock, each ending in a device synchronise, alternated windows; ms per
batch.  `--eager-only` times the loop alone; with `--root DIR` that is the same loop on another
checkout's package (it uses nothing the parent commit lacks).

--align (with --mixed --eval): two BucketedEvalStep over the same stream, both with a hypothesis
log of the whole pass, one with align=True (forced alignment of every head's hypotheses, logged);
whole passes in alternated windows, ms per batch and the per-window difference.

--ensemble (with --mixed --eval): the same pair, one with an ensemble of the five heads decoded
after the two default heads; asserts that the default heads' totals and hypotheses are identical.

--rescore N[:score|mbr] (with --mixed --eval): the same pair, one with rescoring=Rescoring(N, a random
bigram table, lm_weight 0.5, length_bonus 0.2, select) in place of the 1-best decode.  With --fusion a
third pass takes its list from the fused search (Rescoring(..., fusion=True)), in the same alternation.

--mwer (with --mixed): two BucketedTrainStep over the same stream, one with mwer=MWER(0.5, beam_size=--beam)
(the n-best decode, the MWER loss and its backward inside every bucket's graph); whole passes in alternated
windows, ms per step and the per-window difference, and the mean mwer_risk / mwer_loss of the stream.
--mwer-reference / --mwer-lm / --mwer-heads 2 add a third step in the same alternation whose spec has the
reference as a list entry / a bigram table in the posterior / both CTC heads in one grouped call, with the
stream's statistics for that spec.  --ensemble (with --mixed --mwer) puts the five-member ensemble
(MWER(head=EnsembleSpec(...)), its forward and backward inside every bucket's graph) in place of that step's
first head: the figure to compare is the third step's minus the `mwer` step's, which trains the fuse head.
--ensemble-members left,right,body names other members than all five.  --learned adds a fourth step
with the same members in a LearnedEnsemble (weights on the device, d theta in the graph, the parameter in
the optimizer), timed in the same alternated windows.

--distill (with --mixed): BucketedTrainStep with and without distill=Distill(teacher, {left, right, body}):
the fuse head as the teacher, with --ensemble also the five-member ensemble, with --learned also a
LearnedEnsemble; ms per step, the difference to the plain step, the mean ensemble_kd_loss.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch


def _root():
    for i, arg in enumerate(sys.argv):
        if arg == "--root" and i + 1 < len(sys.argv):
            return os.path.abspath(sys.argv[i + 1])
        if arg.startswith("--root="):
            return os.path.abspath(arg.split("=", 1)[1])
    return os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


sys.path.insert(0, _root())


def build(a, dev):
    import scattennet_amd as S
    from scattennet_amd import workloads as W
    w = dict(W.WORKLOADS["cfg3"], B=a.B, T=a.T)
    cfg = W.encoder_cfg(w)
    cfg.update({"self_distillation": True, "distillation_weight": {"left": 0.25, "right": 0.25, "body": 0.25},
                "alignment_module": {"input_size": w["out_fusion"], "hidden_size": 1024, "num_layers": 2,
                                     "dropout": 0.3, "bidirectional": True}})
    torch.manual_seed(0)
    model = S.MSCA_Net(cfg, a.C, device="cuda").to(dev).eval()
    kp, mask, _ = W.synthetic_batch(w, dev, seed=1)
    t4 = W.pooled_frames(w)
    g = torch.Generator().manual_seed(2)
    src = {"keypoints": kp, "mask": mask, "valid_len_in": torch.full((a.B,), t4, device=dev),
           "gloss_labels": torch.randint(1, a.C, (a.B, a.S), generator=g).to(dev),
           "gloss_lengths": torch.randint(a.S // 2, a.S + 1, (a.B,), generator=g).to(dev)}
    return model, src, w, t4


def capture(model, src, check, dev):
    import scattennet_amd as S
    model.check = check
    opt = S.FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.998), weight_decay=1e-3, max_grad_norm=1.0)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            S.train_step(model, opt, src)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.train_step(model, opt, src)
    out = {k: v.detach() for k, v in out.items()}  # the same storage, without the captured autograd graph
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    return graph, out, opt


def window(graph, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        graph.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def scan_alone(a, w, t4, dev):
    import scattennet_amd as S
    shapes = ([(a.B, a.T, w["K_all"], 2)] + [(a.B, t4, w["residual_blocks"][-1])] * 3 + [(a.B, t4, w["out_fusion"])] +
              [(a.B, t4, a.C)] * 5 + [()] * 5)
    ts = [torch.randn(s, device=dev) for s in shapes]
    nbytes = 4 * sum(t.numel() for t in ts)
    S.finite_flags(ts)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(a.scan_reps):
            flags = S.finite_flags(ts)
    graph.replay()
    torch.cuda.synchronize()
    us = sorted(window(graph, 5) * 1e3 / a.scan_reps for _ in range(a.windows))[a.windows // 2]
    assert flags.cpu().tolist() == [0] * len(ts)
    return nbytes, us


def mixed_batches(a, w, dev, n_pool):
    """The seeded stream: [(src_input on the device, T_max)]."""
    import random
    import numpy as np
    from scattennet_amd.data import select_frames
    random.seed(a.seed)
    np.random.seed(a.seed)
    g = torch.Generator().manual_seed(a.seed)
    out = []
    for _ in range(a.batches):
        source = np.random.randint(40, 241, size=a.B)
        lens = [min(len(select_frames(int(n), True, a.T)), a.T) for n in source]  # the rule can draw max_len + 1
        out.append(_batch(a, w, dev, g, lens, n_pool))
    return out


def _batch(a, w, dev, g, lens, n_pool):
    T = max(lens)
    lens_t = torch.tensor(lens)
    mask = (torch.arange(T)[None, :] < lens_t[:, None]).to(torch.int64)
    kp = torch.rand(a.B, T, w["K_all"], 2, generator=g) * mask[:, :, None, None]  # the collator pads with zeros
    vl = lens_t >> n_pool
    gl = torch.minimum((vl // 2).clamp(min=1), torch.randint(a.S // 2, a.S + 1, (a.B,), generator=g))
    src = {"keypoints": kp, "mask": mask, "valid_len_in": vl, "gloss_lengths": gl,
           "gloss_labels": torch.randint(1, a.C, (a.B, a.S), generator=g)}
    return {k: v.to(dev) for k, v in src.items()}, T


def _spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
            "windows": [round(x, 4) for x in v]}


def _pass(fn, batches):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for src, _ in batches:
        fn(src)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def capture_all(step, batches, exact, reset=None):
    """Every graph of a bucketed step captured before anything is timed: a warm-up pass and a
    capture pass over the stream, then batches of exactly a bucket's length (`exact(frames)`) for
    a bucket the stream visits less than twice (or never).  `reset` runs before each pass or
    extra step."""
    for _ in range(2):
        if reset is not None:
            reset()
        _pass(step.step, batches)
    for f in step.frame_buckets:
        while not step.captured(f):
            if reset is not None:
                reset()
            step.step(exact(f))
    assert step.graphs_captured == len(step.frame_buckets)


def mixed(a, dev):
    import scattennet_amd as S
    adam = dict(lr=1e-4, betas=(0.9, 0.998), weight_decay=1e-3, max_grad_norm=1.0)
    model, _, w, _ = build(a, dev)
    model.check = "defer"
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    lengths = [T for _, T in batches]
    opt = S.FusedAdam(model.parameters(), **adam)
    eager = lambda src: S.train_step(model, opt, src)  # noqa: E731
    _pass(eager, batches)  # every shape once
    res = {"workload": "MSCA_Net train_step over a mixed-length stream, eval mode, no report read",
           "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "seed": a.seed, "batch_lengths": lengths}
    if a.eager_only:
        res["eager_ms_per_step"] = _spread([_pass(eager, batches) for _ in range(a.windows)])
        print(json.dumps(res))
        return
    buckets = tuple(int(b) for b in a.buckets.split(","))
    twin, _, _, _ = build(a, dev)
    twin.check = "defer"
    twin_opt = S.FusedAdam(twin.parameters(), capture_slots=len(buckets), **adam)
    bts = S.BucketedTrainStep(twin, twin_opt, a.B, buckets, a.S)
    g = torch.Generator().manual_seed(a.seed + 1)
    capture_all(bts, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0])
    ms = {"eager": [], "bucketed": []}
    for _ in range(a.windows):  # alternated windows
        ms["eager"].append(_pass(eager, batches))
        ms["bucketed"].append(_pass(bts.step, batches))
    res.update({"buckets": list(buckets),
                "bucket_of_batch": [bts.bucket_for(T) for T in lengths],
                "eager_ms_per_step": _spread(ms["eager"]), "bucketed_ms_per_step": _spread(ms["bucketed"]),
                "bucketed_median_below_eager_range": statistics.median(ms["bucketed"]) < min(ms["eager"])})
    # padding overhead per bucket: a batch just above the previous bucket, through the bucket's
    # graph, against a graph captured at exactly that length
    rows, prev = [], 0
    for f in buckets:
        T = prev + 1 if prev else f // 2 + 1
        src, _ = _batch(a, w, dev, g, [T] * a.B, n_pool)
        graph, out, _ = capture(model, src, "defer", dev)
        bts.step(src)
        t = {"bucket_replay": [], "fixed_shape_graph": []}
        for _ in range(a.windows):
            t["fixed_shape_graph"].append(window(graph, a.steps))
            t["bucket_replay"].append(_pass(bts.step, [(src, T)] * a.steps))
        rows.append({"bucket": f, "T": T, "bucket_replay_ms": _spread(t["bucket_replay"]),
                     "fixed_shape_graph_ms": _spread(t["fixed_shape_graph"])})
        del graph, out
        prev = f
    res["padding_overhead"] = rows
    print(json.dumps(res))


def mixed_mwer(a, dev):
    """--mixed --mwer: two BucketedTrainStep over the same stream in alternated windows, one with
    mwer=MWER(0.5, beam_size=--beam) (the n-best decode, the MWER loss and its backward inside the
    graph), and the loss's statistics on the stream: the mean risk, the share of clips whose error
    counts are not all equal (the clips that get a gradient) and the share of non-zero gradient rows,
    from an untimed `mwer_loss` call on each step's own logits (an untrained head: this shows the path
    is exercised, not that MWER lowers WER)."""
    import scattennet_amd as S
    adam = dict(lr=1e-4, betas=(0.9, 0.998), weight_decay=1e-3, max_grad_norm=1.0)
    buckets = tuple(int(b) for b in a.buckets.split(","))
    steps = {}
    variants = [("plain", None), ("mwer", S.MWER(0.5, beam_size=a.beam))]
    if a.mwer_reference or a.mwer_lm or a.mwer_heads > 1 or a.ensemble:
        # a third step with the extended spec: the reference as a list entry, the gloss model's
        # prior (a random normalised table, weight 0.5), the first --mwer-heads CTC heads grouped;
        # --ensemble: the five-member ensemble in place of the first head (its backward in the graph)
        names = ("fuse_coord_gloss_logits", "alignment_gloss_logits")[:max(a.mwer_heads, 1)]
        if a.ensemble:
            from scattennet_amd.model import _LOGITS
            members = tuple(a.ensemble_members.split(",")) if a.ensemble_members else _LOGITS
            names = (S.EnsembleSpec(members),) + names[1:]
        lm = None
        if a.mwer_lm:
            table = torch.log_softmax(torch.randn(a.C, a.C, generator=torch.Generator().manual_seed(a.seed + 7)) * 2, -1)
            lm = S.BigramLM(table, dev)
        variants.append(("mwer_ext", S.MWER(0.5, beam_size=a.beam, reference=a.mwer_reference, lm=lm,
                                            lm_weight=0.5 if a.mwer_lm else 0.0,
                                            head=names if a.mwer_heads > 1 else names[0])))
        if a.ensemble and a.learned:
            # --learned: a fourth step, the same spec with the ensemble's weights learned (a
            # LearnedEnsemble on the device, its parameter in the optimizer, d theta in the graph)
            learned = (S.LearnedEnsemble(members).to(dev),) + names[1:]
            variants.append(("mwer_learned", S.MWER(0.5, beam_size=a.beam, reference=a.mwer_reference, lm=lm,
                                                    lm_weight=0.5 if a.mwer_lm else 0.0,
                                                    head=learned if a.mwer_heads > 1 else learned[0])))
    specs = dict(variants)
    for name, spec in variants:
        model, _, w, _ = build(a, dev)
        model.check = "defer"
        extra = [p for h in (spec.heads if spec else ()) if isinstance(h, S.LearnedEnsemble) for p in h.parameters()]
        opt = S.FusedAdam(list(model.parameters()) + extra, capture_slots=len(buckets), **adam)
        steps[name] = S.BucketedTrainStep(model, opt, a.B, buckets, a.S, mwer=spec)
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    g = torch.Generator().manual_seed(a.seed + 1)
    for step in steps.values():
        capture_all(step, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0])
    ms = {k: [] for k in steps}
    for _ in range(a.windows):  # alternated windows
        for k, step in steps.items():
            ms[k].append(_pass(step.step, batches))
    def stream_statistics(name):
        """The figures of one MWER step over the stream, on its first head."""
        spec = specs[name]
        risk, loss, skipped, clips, live, rows, nonzero = [], [], 0, 0, 0, 0, 0
        for src, _ in batches:
            out = steps[name].step(src)
            rep = S.read_report(out)
            risk.append(rep["mwer_risk"])
            loss.append(rep["mwer_loss"])
            skipped += rep["skipped"]
            # the same list and loss once more on the step's logits, for the per-clip figures
            head = spec.heads[0]  # a logit key, or the EnsembleSpec of --ensemble
            z = (out[head] if isinstance(head, str) else head.compute(out)).detach().clone().requires_grad_(True)
            nb = S.ctc_decode_nbest_device(z, out["input_lengths"], a.beam, a.beam, collapse_repeats=False)
            l, det = S.mwer_loss(z, out["input_lengths"], src["gloss_labels"], src["gloss_lengths"], nbest=nb,
                                 return_details=True, reference=spec.reference, lm=spec.lm, lm_weight=spec.lm_weight,
                                 length_bonus=spec.length_bonus)
            l.backward()
            valid = torch.isfinite(det["loglik"])
            if spec.reference:  # the reference slot counts where it is in the posterior
                valid[:, -1] = det["ref_valid"] != 0
            err = det["errors"].float()
            hi = torch.where(valid, err, err.new_full((), -1e9)).max(1).values
            lo = torch.where(valid, err, err.new_full((), 1e9)).min(1).values
            clips += a.B
            live += int((hi > lo).sum())
            frames = torch.arange(z.shape[1], device=dev)[None, :] < out["input_lengths"][:, None]
            rows += int(frames.sum())
            nonzero += int(((z.grad.abs().amax(-1) > 0) & frames).sum())
            del l, det
        return {"mwer_risk_mean": round(statistics.mean(risk), 4), "mwer_loss_mean": round(statistics.mean(loss), 6),
                "clips_with_non_constant_errors": round(live / clips, 4),
                "gradient_rows_non_zero": round(nonzero / max(rows, 1), 4), "skipped_steps": skipped}

    diff = [x - y for x, y in zip(ms["mwer"], ms["plain"])]
    res = {"workload": "MSCA_Net BucketedTrainStep over a mixed-length stream with and without the MWER "
                       "loss, eval mode, no report read in the timed passes",
           "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "seed": a.seed, "beam": a.beam,
           "buckets": list(buckets), "batch_lengths": [T for _, T in batches],
           "plain_ms_per_step": _spread(ms["plain"]), "mwer_ms_per_step": _spread(ms["mwer"]),
           "mwer_minus_plain_ms_per_step": _spread(diff), **stream_statistics("mwer")}
    if "mwer_ext" in steps:
        res["mwer_ext"] = {"spec": repr(specs["mwer_ext"]), "ms_per_step": _spread(ms["mwer_ext"]),
                           "minus_plain_ms_per_step": _spread([x - y for x, y in zip(ms["mwer_ext"], ms["plain"])]),
                           "minus_mwer_ms_per_step": _spread([x - y for x, y in zip(ms["mwer_ext"], ms["mwer"])]),
                           **stream_statistics("mwer_ext")}
    if "mwer_learned" in steps:
        ens = specs["mwer_learned"].heads[0]
        res["mwer_learned"] = {"spec": repr(specs["mwer_learned"]), "ms_per_step": _spread(ms["mwer_learned"]),
                               "minus_mwer_ext_ms_per_step": _spread([x - y for x, y in zip(ms["mwer_learned"],
                                                                                            ms["mwer_ext"])]),
                               **stream_statistics("mwer_learned"), "weights_after": [round(v, 6) for v in ens.weights()]}
    print(json.dumps(res))


def mixed_distill(a, dev):
    """--mixed --distill: BucketedTrainStep over the same stream in alternated windows, plain and with
    distill=Distill(teacher, {left, right, body}) on top of the model's own distillation terms: the
    teacher is the fuse head (the grouped call at G = 1), with --ensemble the five-member ensemble
    (--ensemble-members names others) formed inside the kernels, with --learned its weights from a
    LearnedEnsemble's scores on the device.  ms per step, the per-window difference to the plain
    step and the mean ensemble_kd_loss over the stream."""
    import scattennet_amd as S
    from scattennet_amd.model import _LOGITS
    adam = dict(lr=1e-4, betas=(0.9, 0.998), weight_decay=1e-3, max_grad_norm=1.0)
    buckets = tuple(int(b) for b in a.buckets.split(","))
    students = {"left": 1.0, "right": 1.0, "body": 1.0}
    variants = [("plain", None), ("distill_head", S.Distill("fuse_coord_gloss_logits", students))]
    if a.ensemble:
        members = tuple(a.ensemble_members.split(",")) if a.ensemble_members else _LOGITS
        variants.append(("distill_ensemble", S.Distill(S.EnsembleSpec(members), students)))
        if a.learned:
            variants.append(("distill_learned", S.Distill(S.LearnedEnsemble(members).to(dev), students)))
    steps = {}
    for name, spec in variants:
        model, _, w, _ = build(a, dev)
        model.check = "defer"
        opt = S.FusedAdam(list(model.parameters()), capture_slots=len(buckets), **adam)
        steps[name] = S.BucketedTrainStep(model, opt, a.B, buckets, a.S, distill=spec)
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    g = torch.Generator().manual_seed(a.seed + 1)
    for step in steps.values():
        capture_all(step, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0])
    ms = {k: [] for k in steps}
    for _ in range(a.windows):  # alternated windows
        for k, step in steps.items():
            ms[k].append(_pass(step.step, batches))
    res = {"workload": "MSCA_Net BucketedTrainStep over a mixed-length stream with and without the ensemble "
                       "distillation term, eval mode, no report read in the timed passes",
           "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "seed": a.seed, "buckets": list(buckets),
           "batch_lengths": [T for _, T in batches], "plain_ms_per_step": _spread(ms["plain"])}
    for name, spec in variants[1:]:
        reps = [S.read_report(steps[name].step(src)) for src, _ in batches]
        res[name] = {"spec": repr(spec), "ms_per_step": _spread(ms[name]),
                     "minus_plain_ms_per_step": _spread([x - y for x, y in zip(ms[name], ms["plain"])]),
                     "ensemble_kd_loss_mean": round(statistics.mean(r["ensemble_kd_loss"] for r in reps), 6),
                     "skipped_steps": sum(r["skipped"] for r in reps)}
    print(json.dumps(res))


def eval_loop(S, model, beam):
    """One batch of the loop a user writes from the parts: returns what it read."""
    def step(src):
        with torch.no_grad():
            out = model(src)
        ref = src["gloss_labels"].to(torch.int32)
        packed = [out["total_loss"].reshape(1).view(torch.int32)]
        for k, v in out.items():
            if "gloss_logits" not in k:
                continue
            tokens, lengths, _ = S.ctc_decode_device(v, out["input_lengths"], beam)
            counts = S.wer_counts(ref, src["gloss_lengths"], tokens, lengths)
            packed += [lengths, tokens.reshape(-1), counts.reshape(-1)]
        return torch.cat(packed).cpu()  # the batch's one host read
    return step


def eval_mixed(a, dev):
    import scattennet_amd as S
    model, _, w, _ = build(a, dev)
    model.check = "defer"
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    lengths = [T for _, T in batches]
    loop = eval_loop(S, model, a.beam)
    _pass(loop, batches)  # every shape once
    res = {"workload": "MSCA_Net evaluation pass over a mixed-length stream (forward, beam decode of the "
                       "gloss heads, WER counts)", "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "beam": a.beam,
           "seed": a.seed, "batch_lengths": lengths}
    if a.eager_only:
        res["loop_ms_per_batch"] = _spread([_pass(loop, batches) for _ in range(a.windows)])
        print(json.dumps(res))
        return
    buckets = tuple(int(b) for b in a.buckets.split(","))
    bes = S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam)
    g = torch.Generator().manual_seed(a.seed + 1)
    capture_all(bes, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0])

    def bucketed_pass():
        bes.state.reset()
        ms = _pass(bes.step, batches)
        return ms, bes.read()  # the pass's one host read (after the timed window's synchronise)

    ms = {"loop": [], "bucketed": []}
    for _ in range(a.windows):  # alternated windows
        ms["loop"].append(_pass(loop, batches))
        t, results = bucketed_pass()
        ms["bucketed"].append(t)
    res.update({"buckets": list(buckets), "bucket_of_batch": [bes.bucket_for(T) for T in lengths],
                "loop_ms_per_batch": _spread(ms["loop"]), "bucketed_ms_per_batch": _spread(ms["bucketed"]),
                "bucketed_median_below_loop_range": statistics.median(ms["bucketed"]) < min(ms["loop"]),
                "results": {k: round(v, 4) for k, v in results.items()}})
    print(json.dumps(res))


def eval_align(a, dev):
    """--mixed --eval --align: the bucketed evaluation pass with and without the forced alignment
    of every hypothesis, both with a hypothesis log of the whole pass, in alternated windows."""
    import scattennet_amd as S
    model, _, w, _ = build(a, dev)
    model.check = "defer"
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    buckets = tuple(int(b) for b in a.buckets.split(","))
    capacity = a.batches * a.B
    steps = {"plain": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity),
             "align": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity, align=True)}
    g = torch.Generator().manual_seed(a.seed + 1)
    for bes in steps.values():
        capture_all(bes, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0], bes.state.reset)
    ms, results = {k: [] for k in steps}, {}
    for _ in range(a.windows):  # alternated windows
        for k, bes in steps.items():
            bes.state.reset()
            ms[k].append(_pass(bes.step, batches))
            results[k] = bes.read()  # the pass's one host read (after the timed window's synchronise)
    same = results["plain"] == results["align"] and steps["plain"].hypotheses() == steps["align"].hypotheses()
    rows = steps["align"].alignments(frame_scale=1 << n_pool)
    diff = [x - y for x, y in zip(ms["align"], ms["plain"])]
    res = {"workload": "MSCA_Net bucketed evaluation pass over a mixed-length stream, with and without the forced "
                       "alignment of every hypothesis (both log the hypotheses)", "B": a.B, "max_len": a.T, "C": a.C,
           "S": a.S, "beam": a.beam, "seed": a.seed, "buckets": list(buckets),
           "batch_lengths": [T for _, T in batches], "plain_ms_per_batch": _spread(ms["plain"]),
           "align_ms_per_batch": _spread(ms["align"]), "align_minus_plain_ms_per_batch": _spread(diff),
           "same_results_and_hypotheses": same, "clips_aligned": len(rows), "infeasible": sum(v is None for r in rows for v in r.values()),
           "results": {k: round(v, 4) for k, v in results["align"].items()}}
    print(json.dumps(res))


def eval_ensemble(a, dev):
    """--mixed --eval --ensemble: the bucketed evaluation pass with and without one ensemble of
    the five heads added to the two default heads, both with a hypothesis log of the whole pass,
    in alternated windows.  The two default heads' totals and hypotheses must not change."""
    import scattennet_amd as S
    from scattennet_amd.model import _LOGITS
    model, _, w, _ = build(a, dev)
    model.check = "defer"
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    buckets = tuple(int(b) for b in a.buckets.split(","))
    capacity = a.batches * a.B
    spec = {"ensemble_gloss_logits": S.EnsembleSpec(_LOGITS)}
    steps = {"plain": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity),
             "ensemble": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity,
                                            ensembles=spec)}
    g = torch.Generator().manual_seed(a.seed + 1)
    for bes in steps.values():
        capture_all(bes, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0], bes.state.reset)
    ms, results, totals = {k: [] for k in steps}, {}, {}
    for _ in range(a.windows):  # alternated windows
        for k, bes in steps.items():
            bes.state.reset()
            ms[k].append(_pass(bes.step, batches))
            results[k] = bes.read()  # the pass's one host read (after the timed window's synchronise)
            totals[k] = bes.state.raw()["totals"][:2].tolist()
    names = ("alignment_", "fuse_coord_")
    hyps = {k: [{n: h[n] for n in names} for h in bes.hypotheses()] for k, bes in steps.items()}
    assert totals["plain"] == totals["ensemble"], "the default heads' totals changed with the ensemble"
    assert hyps["plain"] == hyps["ensemble"], "the default heads' hypotheses changed with the ensemble"
    assert all(results["plain"][n + "wer"] == results["ensemble"][n + "wer"] for n in names)
    diff = [x - y for x, y in zip(ms["ensemble"], ms["plain"])]
    res = {"workload": "MSCA_Net bucketed evaluation pass over a mixed-length stream, with and without one "
                       "five-member ensemble decoded after the two default heads (both log the hypotheses)",
           "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "beam": a.beam, "seed": a.seed, "buckets": list(buckets),
           "batch_lengths": [T for _, T in batches], "plain_ms_per_batch": _spread(ms["plain"]),
           "ensemble_ms_per_batch": _spread(ms["ensemble"]), "ensemble_minus_plain_ms_per_batch": _spread(diff),
           "default_heads_identical": True, "results": {k: round(v, 4) for k, v in results["ensemble"].items()}}
    print(json.dumps(res))


def eval_rescore(a, dev):
    """--mixed --eval --rescore: the bucketed evaluation pass with the 1-best decode and with the
    n-best decode, bigram rescore and selection in its place, both with a hypothesis log of the
    whole pass, in alternated windows."""
    import scattennet_amd as S
    model, _, w, _ = build(a, dev)
    model.check = "defer"
    n_pool = (len(w["residual_blocks"]) + 1) // 2
    batches = mixed_batches(a, w, dev, n_pool)
    buckets = tuple(int(b) for b in a.buckets.split(","))
    capacity = a.batches * a.B
    n, _, select = a.rescore.partition(":")
    lm = S.BigramLM(torch.log_softmax(torch.randn(a.C, a.C, generator=torch.Generator().manual_seed(a.seed)) * 2, -1),
                    device=dev)
    spec = S.Rescoring(int(n), lm, 0.5, 0.2, select=select or "score")
    steps = {"plain": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity),
             "rescored": S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity,
                                            rescoring=spec)}
    if a.fusion:  # a third pass: the list from the fused search, everything after it unchanged
        fspec = S.Rescoring(int(n), lm, 0.5, 0.2, select=select or "score", fusion=True)
        steps["fused"] = S.BucketedEvalStep(model, a.B, buckets, a.S, beam_size=a.beam, capacity=capacity,
                                            rescoring=fspec)
    g = torch.Generator().manual_seed(a.seed + 1)
    for bes in steps.values():
        capture_all(bes, batches, lambda f: _batch(a, w, dev, g, [f] * a.B, n_pool)[0], bes.state.reset)
    ms, results = {k: [] for k in steps}, {}
    for _ in range(a.windows):  # alternated windows
        for k, bes in steps.items():
            bes.state.reset()
            ms[k].append(_pass(bes.step, batches))
            results[k] = bes.read()  # the pass's one host read (after the timed window's synchronise)
    hyps = {k: bes.hypotheses() for k, bes in steps.items()}
    changed = sum(x != y for x, y in zip(hyps["plain"], hyps["rescored"]))
    diff = [x - y for x, y in zip(ms["rescored"], ms["plain"])]
    res = {"workload": "MSCA_Net bucketed evaluation pass over a mixed-length stream, with the 1-best decode and with "
                       "the n-best decode, bigram rescore and selection in its place (both log the hypotheses)",
           "B": a.B, "max_len": a.T, "C": a.C, "S": a.S, "beam": a.beam, "nbest": spec.nbest, "select": spec.select,
           "seed": a.seed, "buckets": list(buckets), "batch_lengths": [T for _, T in batches],
           "plain_ms_per_batch": _spread(ms["plain"]), "rescored_ms_per_batch": _spread(ms["rescored"]),
           "rescored_minus_plain_ms_per_batch": _spread(diff), "clips": len(hyps["plain"]),
           "clips_with_another_hypothesis": changed,
           "results": {k: round(v, 4) for k, v in results["rescored"].items()}}
    if a.fusion:
        res.update({"fused_ms_per_batch": _spread(ms["fused"]),
                    "fused_minus_rescored_ms_per_batch": _spread([x - y for x, y in zip(ms["fused"], ms["rescored"])]),
                    "clips_fused_differs_from_rescored": sum(x != y for x, y in zip(hyps["rescored"], hyps["fused"])),
                    "fused_results": {k: round(v, 4) for k, v in results["fused"].items()}})
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--T", type=int, default=256)
    ap.add_argument("--C", type=int, default=1124)
    ap.add_argument("--S", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--scan-reps", type=int, default=50)
    ap.add_argument("--mixed", action="store_true", help="the mixed-length stream: eager against BucketedTrainStep")
    ap.add_argument("--eager-only", action="store_true", help="with --mixed: time the eager pass alone")
    ap.add_argument("--eval", action="store_true", help="with --mixed: an evaluation pass, loop against "
                                                        "BucketedEvalStep")
    ap.add_argument("--align", action="store_true", help="with --mixed --eval: the bucketed pass with and without "
                                                         "the forced alignment of every hypothesis")
    ap.add_argument("--ensemble", action="store_true", help="with --mixed --eval: the bucketed pass with and without "
                                                            "one five-member ensemble beside the two default heads; "
                                                            "with --mixed --mwer: a third step that trains on it")
    ap.add_argument("--ensemble-members", default=None, help="with --mixed --mwer --ensemble: the members, logit keys "
                                                             "separated by commas (default: all five)")
    ap.add_argument("--learned", action="store_true", help="with --mixed --mwer --ensemble: a fourth step whose "
                                                           "ensemble weights are learned (LearnedEnsemble)")
    ap.add_argument("--fusion", action="store_true", help="with --mixed --eval --rescore: a third pass whose list "
                                                          "comes from the fused search (Rescoring(fusion=True))")
    ap.add_argument("--rescore", default=None, help="with --mixed --eval: N[:score|mbr], the bucketed pass with and "
                                                    "without the rescored n-best decode")
    ap.add_argument("--distill", action="store_true", help="with --mixed: BucketedTrainStep with and without the "
                                                           "ensemble distillation term (--ensemble, --learned: the "
                                                           "teacher), alternated windows")
    ap.add_argument("--mwer", action="store_true", help="with --mixed: BucketedTrainStep with and without the MWER "
                                                        "loss (beam --beam), alternated windows")
    ap.add_argument("--mwer-reference", action="store_true", help="with --mixed --mwer: a third step whose MWER "
                    "spec has the reference as a list entry")
    ap.add_argument("--mwer-lm", action="store_true", help="with --mixed --mwer: the third step's posterior "
                    "includes a bigram table (weight 0.5)")
    ap.add_argument("--mwer-heads", type=int, default=1, choices=(1, 2), help="with --mixed --mwer: the third "
                    "step trains this many CTC heads in one grouped call")
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--buckets", default="64,128,192,256")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--root", default=None, help="import scattennet_amd from this checkout")
    a = ap.parse_args()
    import scattennet_amd as S
    if not torch.cuda.is_available():
        raise SystemExit("model_bench needs a GPU: there is no CPU path to time")
    dev = torch.device("cuda:0")
    if a.mixed:
        if a.eval and a.align:
            return eval_align(a, dev)
        if a.eval and a.ensemble:
            return eval_ensemble(a, dev)
        if a.eval and a.rescore:
            return eval_rescore(a, dev)
        if a.mwer and not a.eval:
            return mixed_mwer(a, dev)
        if a.distill and not a.eval:
            return mixed_distill(a, dev)
        return eval_mixed(a, dev) if a.eval else mixed(a, dev)
    model, src, w, t4 = build(a, dev)
    graphs = {k: capture(model, src, k, dev) for k in ("off", "defer")}
    ms = {k: [] for k in graphs}
    for _ in range(a.windows):  # alternated windows
        for k, (graph, _, _) in graphs.items():
            ms[k].append(window(graph, a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rep = S.read_report(graphs["defer"][1])

    model.check = "sync"
    opt = S.FusedAdam(model.parameters(), lr=1e-4, betas=(0.9, 0.998), weight_decay=1e-3, max_grad_norm=1.0)
    eager = []
    for i in range(3 + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        S.read_report(S.train_step(model, opt, src))  # the report read is the step's one host read
        torch.cuda.synchronize()
        if i >= 3:
            eager.append((time.perf_counter() - t0) * 1e3)
    nbytes, scan_us = scan_alone(a, w, t4, dev)
    scan_ms = med["defer"] - med["off"]
    print(json.dumps({
        "workload": "MSCA_Net train_step (fwd + finite guard + bwd of total_loss + FusedAdam), eval mode",
        "B": a.B, "T": a.T, "T_pooled": t4, "C": a.C, "S": a.S,
        "parameters": sum(p.numel() for p in model.parameters()),
        "graph_off_ms": round(med["off"], 4), "graph_defer_ms": round(med["defer"], 4),
        "graph_off_windows_ms": [round(v, 4) for v in ms["off"]],
        "graph_defer_windows_ms": [round(v, 4) for v in ms["defer"]],
        "eager_sync_ms": round(statistics.median(eager), 4),
        "scan_cost_ms": round(scan_ms, 4), "scan_cost_fraction_of_step": round(scan_ms / med["defer"], 5),
        "scan_bytes": nbytes, "scan_kernel_us": round(scan_us, 3),
        "scan_GBps_cache_resident": round(nbytes / (scan_us * 1e-6) / 1e9, 1),
        "scan_hbm_roofline_us": round(nbytes / 6.3e12 * 1e6, 3),
        "clips_per_s_graph_defer": round(a.B / med["defer"] * 1e3, 1),
        "total_loss": rep["total_loss"], "skipped": rep["skipped"]}))


if __name__ == "__main__":
    main()
