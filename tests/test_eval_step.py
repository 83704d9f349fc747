"""The evaluation step's host side (scattennet_amd/evaluate.py, the grouped decoders and
sca_eval_accumulate of include/scatten.h): entry points, argument validation without a GPU
call, constructor errors, and `results_from_state` — the function `EvalState.read()` uses to
turn the raw state into evaluate_fn's dict — against a plain-Python restatement of the
reference's meters (opt.py:101-128, MetricLogger's global_avg).  CPU only."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import decode_ref as R
from tests.golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sca_ctc_decode_heads_workspace_bytes", "sca_ctc_greedy_decode_heads", "sca_ctc_beam_decode_heads",
                "sca_eval_accumulate")
ERR_ARG = 1
HEADS = ("alignment_gloss_logits", "fuse_coord_gloss_logits")
STUDENTS = ("left", "right", "body")


def _lib():
    from scattennet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        getattr(lib, name).argtypes, getattr(lib, name).restype = _lib.EXPORTS[name]
    return lib


def test_header_library_and_binding_have_the_entry_points():
    from scattennet_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "scatten.h")).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert re.search(r"^\s*\w+\s+%s\s*\(" % name, src, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
        nargs = len(re.search(r"%s\s*\((.*?)\)" % name, src, flags=re.S).group(1).split(","))
        assert len(_lib.EXPORTS[name][0]) == nargs, name
    assert re.search(r"#define SCA_EVAL_MAX_HEADS 8\b", src) and _lib.EVAL_MAX_HEADS == 8
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRY_POINTS:
        assert name in doc, name


def test_struct_layouts_match_header(tmp_path):
    """The ctypes mirrors of sca_decode_heads and sca_eval_state (the state layout the kernels
    write) have the C structs' size and field offsets."""
    from scattennet_amd import _lib as L
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    structs = {"sca_decode_heads": L.DecodeHeads, "sca_eval_state": L.EvalState}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scatten.h"', "int main(void) {"]
    for cs, cls in structs.items():
        lines.append(f'printf("{cs} size %zu\\n", sizeof({cs}));')
        lines += [f'printf("{cs}.{f} %zu\\n", offsetof({cs}, {f}));' for f, _ in cls._fields_]
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line)
    for cs, cls in structs.items():
        assert int(got[f"{cs} size"]) == ctypes.sizeof(cls), cs
        for f, _ in cls._fields_:
            assert int(got[f"{cs}.{f}"]) == getattr(cls, f).offset, (cs, f)
    assert ctypes.sizeof(L.EvalState) % 8 == 0  # cleared and copied as 8-byte words


def test_argument_validation_makes_no_gpu_call():
    """Unsupported sizes are SCA_ERR_ARG before any launch.  The pointers are non-null but
    never dereferenced (a launch with them could not succeed without a device)."""
    from scattennet_amd import _lib as L
    lib = _lib()
    p = ctypes.c_void_p(0x1000)
    hx = L.DecodeHeads()
    for g in range(8):
        hx.logits[g] = 0x1000
    h = ctypes.byref(hx)
    beam = lambda G, B, T, C, W, heads=h: lib.sca_ctc_beam_decode_heads(heads, G, p, B, T, C, W, 1, p, p, p, p, None)  # noqa: E731
    greedy = lambda G, B, T, C, heads=h: lib.sca_ctc_greedy_decode_heads(heads, G, p, B, T, C, p, p, p, p, None)  # noqa: E731
    assert beam(0, 2, 8, 16, 5) == ERR_ARG and beam(9, 2, 8, 16, 5) == ERR_ARG
    assert greedy(0, 2, 8, 16) == ERR_ARG and greedy(9, 2, 8, 16) == ERR_ARG
    assert beam(2, 2, 8, 16, 33) == ERR_ARG and beam(2, 2, 8, 16, 0) == ERR_ARG
    assert beam(2, 2, 8, 8193, 5) == ERR_ARG and greedy(2, 2, 8, 8193) == ERR_ARG
    assert beam(2, 2, 8, 16, 5, None) == ERR_ARG
    hole = L.DecodeHeads()
    hole.logits[0] = 0x1000  # head 1 of G = 2 is null
    assert beam(2, 2, 8, 16, 5, ctypes.byref(hole)) == ERR_ARG and greedy(2, 2, 8, 16, ctypes.byref(hole)) == ERR_ARG
    assert lib.sca_ctc_beam_decode_heads(h, 2, None, 2, 8, 16, 5, 1, p, p, p, p, None) == ERR_ARG  # no in_len
    size = lib.sca_ctc_decode_heads_workspace_bytes
    one = lib.sca_ctc_decode_workspace_bytes
    one.argtypes, one.restype = L.EXPORTS["sca_ctc_decode_workspace_bytes"]
    assert size(0, 8, 64, 1124, 5) == 0 and size(9, 8, 64, 1124, 5) == 0 and size(2, 8, 64, 1124, 33) == 0
    for G in range(1, 9):
        assert size(G, 3, 7, 5, 3) == one(G * 3, 7, 5, 3) > 0  # every (head, clip) has its own slice
    assert size(1, 8, 64, 1124, 5) == one(8, 64, 1124, 5)

    def acc(G=2, B=3, Hmax=13, Rmax=3, nflags=15, nloss=6, capacity=0, width=0, log=None, state=p):
        return lib.sca_eval_accumulate(p, p, G, B, Hmax, p, p, Rmax, p, nflags, nloss, p, state, log, log, capacity,
                                       width, None)
    assert acc(G=0) == ERR_ARG and acc(G=9) == ERR_ARG and acc(B=0) == ERR_ARG
    assert acc(Rmax=129) == ERR_ARG and acc(Hmax=129) == ERR_ARG and acc(Rmax=-1) == ERR_ARG
    assert acc(nflags=65) == ERR_ARG and acc(nloss=12) == ERR_ARG and acc(capacity=-1) == ERR_ARG
    assert acc(capacity=4, width=13, log=None) == ERR_ARG  # a log without its buffers
    assert acc(capacity=4, width=0, log=p) == ERR_ARG
    assert acc(state=None) == ERR_ARG
    with pytest.raises(ValueError, match="sca_eval_accumulate"):
        L.check(acc(G=9), "sca_eval_accumulate")


def test_python_validation_comes_before_the_device():
    import scattennet_amd as S
    x = torch.randn(2, 8, 12)
    il = torch.tensor([8, 8])
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.ctc_decode_heads_device([], il, beam_size=5)
    with pytest.raises(ValueError, match="between 1 and 8"):
        S.ctc_decode_heads_device([x] * 9, il, beam_size=5)
    with pytest.raises(ValueError, match="same shape"):
        S.ctc_decode_heads_device([x, torch.randn(2, 8, 13)], il, beam_size=5)
    with pytest.raises(ValueError, match="same shape"):
        S.ctc_decode_heads_device([x, x.double()], il, beam_size=5)
    with pytest.raises(ValueError, match="beam_size"):
        S.ctc_decode_heads_device([x, x], il, beam_size=33)
    with pytest.raises(RuntimeError, match="one per clip"):
        S.ctc_decode_heads_device([x, x], torch.tensor([8, 8, 8]), beam_size=5)
    with pytest.raises(RuntimeError, match="at most 8"):
        S.ctc_decode_heads_device([x, x], torch.tensor([8, 9]), beam_size=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.ctc_decode_heads_device([x, x], il, beam_size=5)


class _Model:
    """Enough of MSCA_Net for the constructors: cfg, the distillation students, a parameter."""

    def __init__(self, blocks=(64,), maxpos=1024):
        self.cfg = {"residual_blocks": list(blocks), "max_position_embeddings": maxpos}
        self._p = torch.nn.Parameter(torch.zeros(1))

    def _students(self):
        return list(STUDENTS)

    def parameters(self):
        return iter([self._p])


def test_constructor_errors():
    import scattennet_amd as S
    from scattennet_amd import evaluate as E
    m = _Model()  # one pooling stage
    with pytest.raises(ValueError, match="pooled frames"):
        S.BucketedEvalStep(m, 3, (64, 258), 8)  # 258 >> 1 = 129
    with pytest.raises(ValueError, match="label_bucket 129"):
        S.BucketedEvalStep(m, 3, (64, 256), 129)
    with pytest.raises(ValueError, match="multiple of"):
        S.BucketedEvalStep(m, 3, (33,), 8)
    with pytest.raises(ValueError, match="distinct and non-empty"):
        S.BucketedEvalStep(m, 3, (), 8)
    with pytest.raises(ValueError, match="positive"):
        S.BucketedEvalStep(m, 0, (64,), 8)
    assert E.check_eval_buckets(m.cfg, (256, 64), 128) == (64, 256)  # 128 pooled frames and labels fit
    assert E.check_eval_buckets(_Model((64, 64, 64)).cfg, (512,), 8) == (512,)  # two stages: 512 >> 2 = 128
    with pytest.raises(ValueError, match="unknown head"):
        S.EvalState(m, heads=("gloss_logits",))
    with pytest.raises(ValueError, match="distinct"):
        S.EvalState(m, heads=("left", "left"))
    with pytest.raises(ValueError, match="log_width"):
        S.EvalState(m, capacity=4)
    with pytest.raises(ValueError, match="log_width"):
        S.EvalState(m, capacity=4, log_width=129)
    assert E.default_heads() == HEADS
    assert [E.logits_name(k) for k in HEADS] == ["alignment_", "fuse_coord_"]
    st = S.EvalState(m)  # host tensors here: nothing touches a device in the constructor
    assert st.heads == HEADS and st.capacity == 0
    assert st.loss_names == ["alignment_loss", "fuse_coord_loss", "left_distill_loss", "right_distill_loss",
                             "body_distill_loss", "total_loss"]
    assert len(st.flag_names) == 15
    bes = S.BucketedEvalStep(m, 3, (64, 32), 8, capacity=6)
    assert bes.state.log_width == 32 and bes.state.hyp_log.shape == (6, 2, 32) and bes.graphs_captured == 0


# ------------------------------------------------------- read(): evaluate_fn's meters, restated
def _meters(step_losses, refs, hyps_by_head):
    """opt.py:76-128 in plain Python: one SmoothedValue per key (total += value, count += 1,
    global_avg = total / count), wer_list per head over all clips, the minimum from 200."""
    total, count = {}, {}
    for losses in step_losses:
        upd = dict(losses)
        upd["loss"] = losses["total_loss"]
        for k, v in upd.items():
            total[k] = total.get(k, 0.0) + float(v)
            count[k] = count.get(k, 0) + 1
    out = {k: total[k] / count[k] for k in total}
    out["wer"] = 200
    for name, hyps in hyps_by_head.items():
        rate = R.wer_list(refs, hyps)["wer"]
        out[name + "wer"] = rate
        out["wer"] = min(rate, out["wer"])
    return out


def _raw(steps, totals, loss_sum, flags=None, overflow=0, first_flagged=0):
    t = np.zeros((8, 4), np.int32)
    t[:len(totals)] = totals
    ls = np.zeros(11)
    ls[:len(loss_sum)] = loss_sum
    f = [0] * 64
    for i, v in (flags or {}).items():
        f[i] = v
    return {"cursor": 0, "steps": steps, "overflow": overflow, "first_flagged": first_flagged, "totals": t,
            "flags": f, "loss_sum": ls}


def _wer_pairs():
    with np.load(os.path.join(GOLDEN, "wer_cases.npz")) as z:
        N = len(z["counts"])
        refs = [z["ref"][n, :z["ref_len"][n]].tolist() for n in range(N)]
        hyps = [z["hyp"][n, :z["hyp_len"][n]].tolist() for n in range(N)]
        return refs, hyps, z["counts"].astype(np.int64)


def test_results_from_state_matches_the_reference_meters():
    from scattennet_amd import evaluate as E
    from scattennet_amd.model import flag_names
    refs, hyps, counts = _wer_pairs()
    N = len(refs)
    assert N >= 4
    # two heads over the same references: head 0 has the fixture's hypotheses, head 1 the same
    # hypotheses rotated by one clip (other counts, restated below)
    rot = hyps[1:] + hyps[:1]
    totals = [counts.sum(0), np.array([R.wer_single(r, h) for r, h in zip(refs, rot)], np.int64).sum(0)]
    assert totals[0].tolist() == np.array([R.wer_single(r, h) for r, h in zip(refs, hyps)]).sum(0).tolist()
    loss_keys = E.loss_names(STUDENTS)
    rng = np.random.default_rng(0)
    steps = [{k: float(np.float32(rng.uniform(0.1, 40.0))) for k in loss_keys} for _ in range(7)]
    loss_sum = [0.0] * len(loss_keys)
    for s in steps:  # the device's sum: float64, in step order
        for i, k in enumerate(loss_keys):
            loss_sum[i] += s[k]
    got = E.results_from_state(_raw(7, totals, loss_sum), HEADS, loss_keys, flag_names(STUDENTS))
    want = _meters(steps, refs, {"alignment_": hyps, "fuse_coord_": rot})
    assert set(got) == set(want) == set(loss_keys) | {"loss", "wer", "alignment_wer", "fuse_coord_wer"}
    for k in want:
        assert got[k] == want[k], k  # the same float64 operations in the same order: exact
    assert got["wer"] == min(got["alignment_wer"], got["fuse_coord_wer"]) < 200


def test_results_from_state_rules_and_errors():
    from scattennet_amd import evaluate as E
    from scattennet_amd.model import flag_names
    names = flag_names(STUDENTS)
    loss_keys = E.loss_names(STUDENTS)
    # zero totals count as 1: no errors over 5 reference tokens is 1 / 5, no reference tokens 1 / 1
    got = E.results_from_state(_raw(1, [[0, 0, 0, 5], [0, 0, 0, 0]], [1.0] * 6), HEADS, loss_keys, names)
    assert got["alignment_wer"] == R.wer_list([[1, 2, 3, 4, 5]], [[1, 2, 3, 4, 5]])["wer"] == 20.0
    assert got["fuse_coord_wer"] == R.wer_list([[]], [[]])["wer"] == 100.0 and got["wer"] == 20.0
    # every head above 200: the minimum keeps its start value
    got = E.results_from_state(_raw(1, [[0, 30, 0, 10], [0, 50, 0, 10]], [1.0] * 6), HEADS, loss_keys, names)
    assert got["alignment_wer"] == 300.0 and got["wer"] == 200
    # any subset of heads, in the state's order
    got = E.results_from_state(_raw(2, [[1, 0, 0, 4]], [3.0] * 6), ("left",), loss_keys, names)
    assert got["leftwer"] == 25.0 and got["wer"] == 25.0 and got["loss"] == 1.5
    with pytest.raises(RuntimeError, match="overflowed"):
        E.results_from_state(_raw(3, [[0, 0, 0, 1]] * 2, [1.0] * 6, overflow=1), HEADS, loss_keys, names)
    with pytest.raises(RuntimeError, match="longer than"):
        E.results_from_state(_raw(3, [[0, 0, 0, 1]] * 2, [1.0] * 6, overflow=2), HEADS, loss_keys, names)
    with pytest.raises(RuntimeError, match="no step"):
        E.results_from_state(_raw(0, [[0, 0, 0, 0]] * 2, [0.0] * 6), HEADS, loss_keys, names)
    with pytest.raises(ValueError, match="^NaN or inf in input keypoints$"):
        E.results_from_state(_raw(3, [[0, 0, 0, 1]] * 2, [1.0] * 6, flags={0: 1, 9: 2}, first_flagged=2), HEADS,
                             loss_keys, names)
    with pytest.raises(ValueError, match="^inf in fuse_coord_gloss_logits$"):
        E.results_from_state(_raw(3, [[0, 0, 0, 1]] * 2, [1.0] * 6, flags={9: 2}, first_flagged=1), HEADS, loss_keys,
                             names)
    # the flag error comes first: a flagged pass is not reported as an overflow
    with pytest.raises(ValueError, match="NaN in left"):
        E.results_from_state(_raw(3, [[0, 0, 0, 1]] * 2, [1.0] * 6, flags={6: 1}, overflow=1, first_flagged=3),
                             HEADS, loss_keys, names)
