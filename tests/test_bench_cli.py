"""bench.py's command line: a plain run is the timed steps and the result line only, --steps
sets the number of timed steps, and --dump-outputs writes what the last timed step computed.

bench.py is always started as a process of its own (it configures the HIP runtime through the
environment before torch initialises it, which must not leak into the test process).
"""
import json
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_large_arrays_reproducibly(tmp_path):
    """Over the byte budget every array gets an equal share: small arrays whole, large ones a
    fixed sample (same positions on every call, in index order); under it, everything whole."""
    code = textwrap.dedent("""
        import sys, torch
        import bench
        class P:
            def __init__(self, t): self.grad = t
        bench.DUMP_BUDGET_BYTES = 4 * 4000
        outs = [torch.arange(6000, dtype=torch.float32).reshape(60, 100), torch.arange(7, dtype=torch.float64)]
        named = [("big", P(torch.arange(5000, dtype=torch.float32) * 2)), ("small", P(torch.ones(3))),
                 ("unused", P(None))]
        bench.dump_outputs(sys.argv[1], outs, named)
        bench.dump_outputs(sys.argv[2], outs, named)
        bench.DUMP_BUDGET_BYTES = 4 * 20000
        bench.dump_outputs(sys.argv[3], outs, named)
    """)
    dirs = [str(tmp_path / n) for n in ("a", "b", "whole")]
    subprocess.run([sys.executable, "-c", code] + dirs, cwd=ROOT, check=True, timeout=120)
    names = sorted(os.listdir(dirs[0]))
    assert names == ["grad.big.npy", "grad.small.npy", "out0.npy", "out1.npy"]
    a = {n: np.load(os.path.join(dirs[0], n)) for n in names}
    b = {n: np.load(os.path.join(dirs[1], n)) for n in names}
    assert sum(x.nbytes for x in a.values()) <= 4 * 4000
    for n in names:
        assert a[n].dtype == np.float32 and np.array_equal(a[n], b[n]), n
    assert np.array_equal(a["grad.small.npy"], np.ones(3)) and np.array_equal(a["out1.npy"], np.arange(7))
    for n, step, size in (("out0.npy", 1, 6000), ("grad.big.npy", 2, 5000)):
        pos = a[n] / step  # the values are step * position
        assert a[n].shape == (1000,) and np.all(np.diff(pos) > 0) and pos.max() < size, n
    assert not np.array_equal(a["out0.npy"][:1000], np.arange(1000))  # a sample, not the head
    whole = {n: np.load(os.path.join(dirs[2], n)) for n in names}
    assert whole["out0.npy"].shape == (60, 100) and whole["grad.big.npy"].shape == (5000,)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """config 1 (one small stream): the result line's fields, --steps honoured, nothing of
    --full in a plain run, and the dumped arrays equal to an eager forward + backward of the
    same seeded model and batch here (the same kernels on the same inputs, eager against a
    graph replay: 1e-5 of the largest output / gradient magnitude covers any fp32 reordering)."""
    from scattennet_amd import workloads as W
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "cfg1", "--steps", "3",
                        "--warmup", "1", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "clips/s" and line["dtype"] == "fp32"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    w = W.WORKLOADS["cfg1"]
    assert line["value"] == pytest.approx(w["B"] * 1000.0 / line["ms_per_step"], rel=1e-3)
    assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None

    dev = torch.device("cuda:0")
    model = W.build_streams(w, dev, seed=0, init="reference")
    kp, mask, gout = W.synthetic_batch(w, dev, seed=1)
    outs = model(kp, mask)
    torch.autograd.backward(outs, [gout[g].contiguous() for g in range(gout.shape[0])])
    torch.cuda.synchronize()
    want = {f"out{g}": o.detach() for g, o in enumerate(outs)}
    want.update({f"grad.{n}": p.grad for n, p in model.named_parameters() if p.grad is not None})
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in want)
    # gradients on the scale of the largest one (some are zero up to roundoff, e.g. key biases)
    scale = {"out": max(float(t.abs().max()) for n, t in want.items() if n.startswith("out")),
             "gra": max(float(t.abs().max()) for n, t in want.items() if n.startswith("grad."))}
    total = 0
    for n, t in want.items():
        got = np.load(out / (n + ".npy"))
        total += got.nbytes
        assert got.dtype == np.float32 and got.shape == tuple(t.shape), n
        assert np.abs(got - t.cpu().numpy()).max() <= 1e-5 * scale[n[:3]], n
    assert total <= 64 * 2 ** 20
