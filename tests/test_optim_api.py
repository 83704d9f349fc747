"""scattennet_amd.optim without a GPU: constructor contracts, the scheduler against the
reference's recorded rates, build_optimizer's groups, the chunk planner and the header."""
import os
import re

import numpy as np
import pytest
import torch

from tests.golden_util import load_arrays, manifest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _param(*shape):
    return torch.nn.Parameter(torch.zeros(*shape))


@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(0.9, 1.0)),
                                dict(betas=(-0.1, 0.9)), dict(weight_decay=-1e-3), dict(max_grad_norm=0.0),
                                dict(max_grad_norm=-1.0)])
def test_constructor_rejects_bad_hyperparameters(kw):
    from scattennet_amd import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam([_param(4)], **kw)
    torch_kw = {k: v for k, v in kw.items() if k != "max_grad_norm"}
    if torch_kw:  # the same values are refused by torch.optim.Adam, with the same message
        with pytest.raises(ValueError) as ours:
            FusedAdam([_param(4)], **torch_kw)
        with pytest.raises(ValueError) as theirs:
            torch.optim.Adam([_param(4)], **torch_kw)
        assert str(ours.value) == str(theirs.value)


def test_constructor_rejects_empty_and_non_tensor_params():
    from scattennet_amd import FusedAdam
    with pytest.raises(ValueError):
        FusedAdam([])
    with pytest.raises(TypeError):
        FusedAdam([3.0])


@pytest.mark.parametrize("kw", [dict(maximize=True), dict(foreach=True), dict(capturable=True),
                                dict(differentiable=True), dict(fused=True)])
def test_unsupported_keywords_raise_type_error(kw):
    from scattennet_amd import FusedAdam
    with pytest.raises(TypeError):
        FusedAdam([_param(4)], **kw)
    with pytest.raises(TypeError):  # ... and as a per-group option
        FusedAdam([dict(params=[_param(4)], **kw)])


def test_non_fp32_and_non_contiguous_parameters_raise():
    from scattennet_amd import FusedAdam
    with pytest.raises(ValueError, match="fp32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))])
    with pytest.raises(ValueError, match="fp32"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    with pytest.raises(ValueError, match="contiguous"):
        FusedAdam([torch.nn.Parameter(torch.zeros(4, 6).t())])


def test_param_groups_have_adams_keys_and_per_group_options():
    from scattennet_amd import FusedAdam
    a, b = _param(3), _param(5)
    ours = FusedAdam([dict(params=[a], lr=0.5, weight_decay=0.1), dict(params=[b])], lr=0.002, betas=(0.9, 0.998))
    theirs = torch.optim.Adam([dict(params=[a], lr=0.5, weight_decay=0.1), dict(params=[b])], lr=0.002,
                              betas=(0.9, 0.998))
    assert [set(g) for g in ours.param_groups] == [set(g) for g in theirs.param_groups]
    for go, gt in zip(ours.param_groups, theirs.param_groups):
        assert {k: v for k, v in go.items() if k != "params"} == {k: v for k, v in gt.items() if k != "params"}
    assert ours.state_dict()["param_groups"] == theirs.state_dict()["param_groups"]


def test_step_on_cpu_parameters_raises_no_cpu_fallback():
    from scattennet_amd import FusedAdam, clip_grad_norm_
    p = _param(8)
    p.grad = torch.ones(8)
    opt = FusedAdam([p], lr=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(8)) and len(opt.state) == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        clip_grad_norm_([p], 1.0)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([p], 1.0, norm_type=1.0)
    with pytest.raises(ValueError, match="norm_type"):
        clip_grad_norm_([p], 1.0, norm_type=float("inf"))


def _yaml_section():
    return dict(manifest("manifest_optim.json")["config"])


def test_scheduler_equals_reference_schedule():
    from scattennet_amd import FusedAdam, WarmupCosineAnnealingScheduler
    from torch.optim.lr_scheduler import _LRScheduler
    man = manifest("manifest_optim.json")
    cfg = _yaml_section()
    want = load_arrays("optim_schedule")["lr"]
    assert want.dtype == np.float64 and want.shape == (100, 2)
    opt = FusedAdam([dict(params=[_param(2)], lr=g["lr"]) for g in man["groups"]], lr=cfg["learning_rate"]["default"])
    sched = WarmupCosineAnnealingScheduler(opt, total_epochs=cfg["total_epochs"], warmup_ratio=cfg["warmup_ratio"],
                                           eta_min=cfg["eta_min"])
    assert isinstance(sched, _LRScheduler)
    assert sched.warmup_epochs == 20
    got = []
    for _ in range(cfg["total_epochs"]):
        got.append([g["lr"] for g in opt.param_groups])
        opt._opt_called = True  # no optimizer step happens here: silence the call-order warning
        sched.step()
    got = np.array(got, dtype=np.float64)
    assert np.array_equal(got, want), np.abs(got - want).max()
    # the checkpoint round trip main.py:187-210 relies on
    again = WarmupCosineAnnealingScheduler(opt, total_epochs=cfg["total_epochs"], warmup_ratio=cfg["warmup_ratio"],
                                           eta_min=cfg["eta_min"])
    again.load_state_dict(sched.state_dict())
    assert again.last_epoch == sched.last_epoch and "optimizer" not in sched.state_dict()


class _Bag(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self.items = torch.nn.ParameterList([_param(*s) for s in shapes])


def _toy(layout):
    m = torch.nn.Module()
    for name, shapes in layout.items():
        m.add_module(name, _Bag(shapes))
    return m


def test_build_optimizer_groups_rates_and_errors():
    from scattennet_amd import FusedAdam, build_optimizer
    man = manifest("manifest_optim.json")
    cfg = _yaml_section()
    cfg["learning_rate"] = dict(cfg["learning_rate"], **man["lr_override"])
    model = _toy(man["layout"])
    before = {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items()}
    opt = build_optimizer(cfg, model)
    assert cfg == before  # the config is left as it was
    assert isinstance(opt, FusedAdam) and isinstance(opt, torch.optim.Optimizer)
    assert len(opt.param_groups) == len(man["groups"]) == 2
    for g, want, child in zip(opt.param_groups, man["groups"], model.children()):
        assert g["lr"] == want["lr"] and list(g["betas"]) == want["betas"] and g["eps"] == want["eps"]
        assert g["weight_decay"] == want["weight_decay"] and g["amsgrad"] == want["amsgrad"]
        assert [id(p) for p in g["params"]] == [id(p) for p in child.parameters()]
    assert [g["lr"] for g in opt.param_groups] == [0.0005, 0.002]
    assert sorted(k for k in opt.param_groups[0] if k != "params") == man["group_keys"]
    assert isinstance(build_optimizer(dict(cfg, optimizer="AdamW"), model), FusedAdam)
    assert build_optimizer(dict(cfg, optimizer="adam"), model, max_grad_norm=1.0).max_grad_norm == 1.0
    for name in ("adagrad", "adadelta", "rmsprop", "sgd"):
        with pytest.raises(ValueError, match="not available on the HIP path"):
            build_optimizer(dict(cfg, optimizer=name), model)
    with pytest.raises(ValueError, match="Unknown optimizer lion"):
        build_optimizer(dict(cfg, optimizer="lion"), model)


@pytest.mark.parametrize("chunk", [1, 7, 64, 8192])
def test_chunk_planner_covers_every_element_once(chunk):
    from scattennet_amd.optim import plan_chunks
    numels = [1, 3, 5, 0, 257, 4097, 8192, 8193, 258 * 64, 8199, 16384, 2]
    plan = plan_chunks(numels, chunk)
    seen = [np.zeros(n, dtype=np.int32) for n in numels]
    for t, ln, off in zip(plan["tensor"], plan["len"], plan["offset"]):
        assert 0 < ln <= chunk and off % chunk == 0
        assert 0 <= off and off + ln <= numels[t]  # inside one tensor
        seen[t][off:off + ln] += 1
    assert all((s == 1).all() for s in seen)
    assert len(plan) == sum(-(-n // chunk) for n in numels)
    order = list(zip(plan["tensor"].tolist(), plan["offset"].tolist()))
    assert order == sorted(order)  # a fixed order: by tensor, then by offset
    assert len(plan_chunks([], chunk)) == 0


def test_chunk_planner_large_tensor_offsets_are_64_bit():
    from scattennet_amd.optim import plan_chunks
    plan = plan_chunks([3, 2 ** 31 + 5], 2 ** 20)
    assert plan["offset"].dtype == np.int64
    assert int(plan["offset"][-1]) + int(plan["len"][-1]) == 2 ** 31 + 5 and int(plan["len"][-1]) == 5


def test_header_declares_the_optimizer_entry_points():
    from scattennet_amd import _lib
    src = open(os.path.join(ROOT, "include", "scatten.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("sca_optim_grad_sqnorm", "sca_optim_adam_step", "sca_optim_scale_grads", "sca_optim_blocks",
                 "sca_optim_upload"):
        assert re.search(r"^int\s+" + name + r"\s*\(", src, flags=re.M), name
        assert name in _lib.EXPORTS
    for struct in ("sca_optim_tensor", "sca_optim_chunk", "sca_optim_group", "sca_optim_state"):
        assert re.search(r"\}\s*" + struct + r"\s*;", src), struct


def test_optimizer_struct_mirrors_match_header(tmp_path):
    """tests/test_capi.py checks the mirrors it lists; the optimizer's tables are checked
    here the same way (sizes and field offsets from the header, compiled with the host cc)."""
    import ctypes
    import shutil
    import subprocess
    from scattennet_amd import _lib as L
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    structs = {"sca_optim_tensor": "OptimTensor", "sca_optim_chunk": "OptimChunk", "sca_optim_group": "OptimGroup",
               "sca_optim_state": "OptimState"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "scatten.h"', "int main(void) {"]
    for cs, py in structs.items():
        lines.append(f'printf("{py} size %zu\\n", sizeof({cs}));')
        for f, _ in getattr(L, py)._fields_:
            lines.append(f'printf("{py}.{f} %zu\\n", offsetof({cs}, {f}));')
    lines.append("return 0; }")
    (tmp_path / "layout.c").write_text("\n".join(lines))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.rsplit(" ", 1) for line in out.split("\n") if line)
    for py in structs.values():
        cls = getattr(L, py)
        assert int(got[f"{py} size"]) == ctypes.sizeof(cls), py
        for f, _ in cls._fields_:
            assert int(got[f"{py}.{f}"]) == getattr(cls, f).offset, (py, f)


def test_library_validates_optimizer_arguments():
    """Pure argument checks of the C entry points — no GPU call is made."""
    import ctypes
    from scattennet_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert lib.sca_optim_blocks(0, 10 ** 6) == 2048 and lib.sca_optim_blocks(3, 10) == 3
    assert lib.sca_optim_blocks(0, 5) == 5 and lib.sca_optim_blocks(0, 0) == 1
    assert lib.sca_optim_grad_sqnorm(None, None, 4, 0, None, None, None, None) == 1
    assert lib.sca_optim_adam_step(None, None, -1, None, 0, ctypes.c_float(1.0), None, None, None) == 1
    assert lib.sca_optim_scale_grads(None, None, 4, 0, ctypes.c_float(1.0), None, None, None) == 1
    assert lib.sca_optim_upload(None, None, ctypes.c_long(16), None) == 1
