"""MSCA_Net as a drop-in module: state_dict layout against the reference fixture, constructor
attributes, the no-fallback rule, the flag-words -> ValueError mapping, and the conditions
the whole-model fixture was generated under.  CPU only."""
import copy

import numpy as np
import pytest
import torch

from tests.golden_util import load, load_arrays, manifest

LOGITS = ["alignment_gloss_logits", "left", "right", "body", "fuse_coord_gloss_logits"]


def _fixture():
    return load("model_small", "manifest_model.json")


def _model(fx, **over):
    import scattennet_amd as S
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    cfg.update(over)
    return S.MSCA_Net(cfg, list(range(fx["meta"]["vocab"])))


def test_state_dict_matches_reference_and_loads_strictly():
    fx = _fixture()
    m = _model(fx)
    sd = m.state_dict()
    assert list(sd.keys()) == list(fx["param"].keys())  # same keys, same order
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in fx["param"].items()}
    assert sum(v.numel() for v in sd.values()) == fx["meta"]["params"]
    m.load_state_dict(fx["param"], strict=True)
    assert all(torch.equal(v, fx["param"][k]) for k, v in m.state_dict().items())
    assert [n for n, _ in m.named_children()] == ["body_encoder", "left_encoder", "right_encoder",
                                                  "coordinates_fusion", "recognition_head", "loss_fn",
                                                  "distillation_loss"]  # the reference's, in its order


def test_constructor_attributes():
    import scattennet_amd as S
    fx = _fixture()
    cfg = copy.deepcopy(fx["meta"]["cfg"])
    tok = list(range(7))
    m = S.MSCA_Net(cfg, tok, device="cuda")
    assert m.cfg is cfg and cfg["fuse_idx"] == cfg["left_idx"] + cfg["right_idx"] + cfg["body_idx"]
    assert m.device == "cuda" and m.left_idx == cfg["left_idx"] and m.gloss_tokenizer is tok
    assert m.self_distillation is True and m.gradient_clip_val == 1.0 and m.check == "sync"
    assert isinstance(m.loss_fn, torch.nn.CTCLoss) and m.loss_fn.zero_infinity and m.loss_fn.reduction == "none"
    assert isinstance(m.distillation_loss, S.SeqKD)
    assert m.recognition_head.fuse_coord_classifier.out_features == 7
    cfg2 = copy.deepcopy(fx["meta"]["cfg"])
    cfg2["gradient_clip_val"] = 0.5
    m2 = S.MSCA_Net(cfg2, 9)  # an int vocabulary size, as RecognitionHead allows
    assert m2.gradient_clip_val == 0.5 and m2.recognition_head.left_gloss_classifier.out_features == 9
    # _init_weights: xavier Linear with zero bias, LayerNorm (1, 0)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Linear):
            assert float(mod.bias.detach().abs().max()) == 0.0
        elif isinstance(mod, torch.nn.LayerNorm):
            assert float((mod.weight.detach() - 1).abs().max()) == 0.0 and float(mod.bias.detach().abs().max()) == 0.0


def test_forward_on_cpu_tensors_is_refused():
    fx = _fixture()
    m = _model(fx).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(dict(fx["in"]))


def test_bad_check_mode_is_refused():
    fx = _fixture()
    m = _model(fx)
    m.check = "later"
    with pytest.raises(ValueError, match="check"):
        m(dict(fx["in"]))


def test_finite_flags_refuses_cpu_tensors():
    import scattennet_amd as S
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.finite_flags([torch.zeros(4)])


def test_first_error_follows_the_reference_order():
    from scattennet_amd.model import FLAG_INF, FLAG_NAN, first_error, flag_names, report_layout
    names = flag_names(["left", "right", "body"])
    assert names == (["keypoints", "body_embed", "left_embed", "right_embed", "fuse_embed"] + LOGITS +
                     ["alignment_loss", "fuse_coord_loss", "left_distill_loss", "right_distill_loss",
                      "body_distill_loss"])

    def flags(**kw):
        return [kw.get(n, 0) for n in names]

    assert first_error(flags(), names) is None
    assert first_error(flags(left=FLAG_NAN, body_embed=FLAG_NAN), names) == "NaN or inf in body_embed"
    assert first_error(flags(right=FLAG_INF), names) == "inf in right"
    assert first_error(flags(left=FLAG_NAN | FLAG_INF), names) == "NaN in left"
    assert first_error(flags(keypoints=FLAG_INF, fuse_embed=FLAG_NAN), names) == "NaN or inf in input keypoints"
    assert first_error(flags(left_embed=FLAG_INF, right_embed=FLAG_NAN), names) == "NaN or inf in left_embed"
    assert first_error(flags(fuse_embed=FLAG_INF, alignment_gloss_logits=FLAG_NAN), names) == "NaN or inf in fuse_embed"
    assert first_error(flags(alignment_gloss_logits=FLAG_INF, left=FLAG_NAN), names) == "inf in alignment_gloss_logits"
    assert first_error(flags(fuse_coord_gloss_logits=FLAG_NAN, alignment_loss=FLAG_NAN), names) == \
        "NaN in fuse_coord_gloss_logits"
    assert first_error(flags(alignment_loss=FLAG_INF, fuse_coord_loss=FLAG_NAN), names) == "NaN or inf in alignment_loss"
    assert first_error(flags(fuse_coord_loss=FLAG_NAN, left_distill_loss=FLAG_NAN), names) == \
        "NaN or inf in fuse_coord_loss"
    assert first_error(flags(right_distill_loss=FLAG_NAN, body_distill_loss=FLAG_INF), names) == \
        "NaN or inf in right_distill_loss"
    assert first_error(torch.tensor(flags(body=FLAG_INF), dtype=torch.int32), names) == "inf in body"
    lay = report_layout(["left", "right", "body"])
    assert lay["flags"] == (0, 15) and lay["alignment_loss"] == 15 and lay["fuse_coord_loss"] == 16
    assert lay["left_distill_loss"] == 17 and lay["total_loss"] == 20 and lay["guard"] == 21 and lay["words"] == 22
    assert report_layout([])["guard"] == 15 and len(flag_names()) == 12


def test_fixture_conditions_hold_on_the_committed_arrays():
    """What the parity tests rest on: losses below their clamps, logits strictly inside +-50,
    finite per-sample CTC losses, an active clip at every recorded training step."""
    man = manifest("manifest_model.json")["fixtures"]
    meta, steps = man["model_small"], man["model_train_steps"]
    z = load_arrays("model_small")
    assert meta["files"] <= 4 and all(meta["conditions"].values())
    for k in LOGITS:
        assert float(np.abs(z["out." + k]).max()) < 50.0
        assert z["out." + k].shape == (meta["B"], meta["T"] // 2, meta["vocab"])
    assert 0.0 < float(z["out.alignment_loss"]) < 100.0 and 0.0 < float(z["out.fuse_coord_loss"]) < 100.0
    total = float(z["out.fuse_coord_loss"])
    for s in meta["cfg"]["distillation_weight"]:
        v = float(z[f"out.{s}_distill_loss"])
        assert abs(v) < 100.0
        total += v
    assert abs(total - float(z["out.total_loss"])) < 1e-5 * abs(total)
    for k, nll in meta["per_sample_ctc"].items():
        assert len(nll) == meta["B"] and all(np.isfinite(nll))
    assert np.array_equal(z["out.input_lengths"], z["in.valid_len_in"])
    grads = {k[len("grad.param."):] for k in z if k.startswith("grad.param.")}
    params = {k[len("param."):] for k in z if k.startswith("param.")}
    assert grads | set(meta["no_grad"]) == params and not grads & set(meta["no_grad"])
    assert meta["no_grad"] and all(k.startswith("recognition_head.fuse_alignment_head.") for k in meta["no_grad"])
    assert len(z["train.total_loss"]) == steps["steps"] == 6
    assert (z["train.grad_norm"] > steps["clip"]).all() and steps["clip_active_every_step"]
    assert abs(float(z["train.total_loss"][0]) - float(z["out.total_loss"])) < 1e-5 * abs(total)
    rel = max(np.abs(z["train.total_loss"] - z["train.total_loss_fp64"]).max() / np.abs(z["train.total_loss_fp64"]).max(),
              np.abs(z["train.grad_norm"] - z["train.grad_norm_fp64"]).max() / np.abs(z["train.grad_norm_fp64"]).max())
    assert rel <= steps["fp64_vs_fp32_rel"] * (1 + 1e-9) < 1e-3  # the floor lies below the tests' 1e-3


def test_guard_entry_points_validate_their_arguments():
    """Pure argument checks of the C ABI — they return before any GPU call is made."""
    import ctypes

    from scattennet_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)

    def scan(ptrs, numels, flags=p):
        n = len(ptrs)
        return lib.sca_finite_scan(n, (ctypes.c_void_p * max(n, 1))(*ptrs), (ctypes.c_long * max(n, 1))(*numels),
                                   flags, None)

    assert scan([], []) == 0                                   # nothing to scan
    assert scan([p] * (L.GUARD_MAX_TENSORS + 1), [1] * (L.GUARD_MAX_TENSORS + 1)) == 1
    assert scan([None], [3]) == 1 and scan([p], [-1]) == 1 and scan([p + 2], [1]) == 1
    assert scan([p], [4], flags=None) == 1
    assert lib.sca_finite_scan(-1, None, None, None, None) == 1
    with pytest.raises(ValueError, match="sca_finite_scan"):
        L.check(scan([None], [3]), "sca_finite_scan")
    terms = (ctypes.c_void_p * 1)(p)
    assert lib.sca_step_report(None, 4, p, None, 0, None, None, p, None) == 1      # no fuse_coord_loss
    assert lib.sca_step_report(None, 4, p, p, 0, None, None, None, None) == 1      # no report buffer
    assert lib.sca_step_report(None, L.REPORT_MAX_FLAGS + 1, p, p, 0, None, None, p, None) == 1
    assert lib.sca_step_report(None, 4, p, p, L.REPORT_MAX_DISTILL + 1, terms, None, p, None) == 1
    assert lib.sca_step_report(None, 4, p, p, 1, (ctypes.c_void_p * 1)(None), None, p, None) == 1
