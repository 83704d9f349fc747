"""Length buckets, host side: `pad_batch`, the bucket choice and the constructor checks of
`BucketedTrainStep` (all of which run before anything touches the device).  CPU only."""
import copy

import pytest
import torch


def _batch(B=3, T=5, K=4, S=3, concat=False):
    g = torch.Generator().manual_seed(1)
    lengths = torch.tensor([3, 2, 1][:B])
    labels = torch.randint(1, 9, (B, S), generator=g)
    if concat:
        labels = torch.cat([labels[b, :int(lengths[b])] for b in range(B)])
    return {"keypoints": torch.randn(B, T, K, 2, generator=g), "mask": torch.ones(B, T, dtype=torch.int64),
            "valid_len_in": torch.tensor([T // 2] * B), "gloss_labels": labels, "gloss_lengths": lengths,
            "name": ["a", "b", "c"][:B]}


def test_pad_batch_shapes_and_valid_frames():
    import scattennet_amd as S
    src = _batch()
    before = {k: v.clone() if torch.is_tensor(v) else list(v) for k, v in src.items()}
    out = S.pad_batch(src, 8, 6)
    assert out["keypoints"].shape == (3, 8, 4, 2) and out["mask"].shape == (3, 8)
    assert out["keypoints"].dtype == torch.float32 and out["mask"].dtype == torch.int64
    assert torch.equal(out["keypoints"][:, :5], src["keypoints"]) and not out["keypoints"][:, 5:].any()
    assert torch.equal(out["mask"][:, :5], src["mask"]) and not out["mask"][:, 5:].any()
    assert out["gloss_labels"].shape == (3, 6)
    assert torch.equal(out["gloss_labels"][:, :3], src["gloss_labels"]) and not out["gloss_labels"][:, 3:].any()
    assert out["valid_frames"].dtype == torch.int32 and out["valid_frames"].tolist() == [5]
    assert out["valid_len_in"] is src["valid_len_in"] and out["gloss_lengths"] is src["gloss_lengths"]
    assert out["name"] == src["name"]
    # the input dict and its tensors are as they were
    assert set(src) == set(before) and "valid_frames" not in src
    for k, v in before.items():
        assert torch.equal(src[k], v) if torch.is_tensor(v) else src[k] == v


def test_pad_batch_exact_fit_and_no_label_bucket():
    import scattennet_amd as S
    src = _batch()
    out = S.pad_batch(src, 5)
    assert torch.equal(out["keypoints"], src["keypoints"]) and out["valid_frames"].tolist() == [5]
    assert out["gloss_labels"] is src["gloss_labels"]  # labels=None: left alone


def test_pad_batch_concatenated_labels():
    import scattennet_amd as S
    two_d = _batch()
    src = _batch(concat=True)
    assert src["gloss_labels"].dim() == 1 and src["gloss_labels"].numel() == 6
    out = S.pad_batch(src, 6, 4)
    assert out["gloss_labels"].shape == (3, 4)
    for b, n in enumerate([3, 2, 1]):
        assert torch.equal(out["gloss_labels"][b, :n], two_d["gloss_labels"][b, :n])
        assert not out["gloss_labels"][b, n:].any()


def test_pad_batch_errors():
    import scattennet_amd as S
    with pytest.raises(ValueError, match="5 frames"):
        S.pad_batch(_batch(), 4)
    with pytest.raises(ValueError, match="3 labels"):
        S.pad_batch(_batch(), 8, 2)
    with pytest.raises(ValueError, match="3 labels"):
        S.pad_batch(_batch(concat=True), 8, 2)


def test_bucket_choice():
    from scattennet_amd.bucketed import pick_bucket
    buckets = (64, 128, 192)
    assert pick_bucket(buckets, 64) == 64       # exact fit
    assert pick_bucket(buckets, 65) == 128      # the one above
    assert pick_bucket(buckets, 1) == 64
    assert pick_bucket(buckets, 192) == 192
    with pytest.raises(ValueError, match="193 frames fits no bucket"):
        pick_bucket(buckets, 193)


class _Model:
    """Only what the constructor may look at before it touches the device."""

    def __init__(self, blocks, maxpos):
        self.cfg = {"residual_blocks": blocks, "max_position_embeddings": maxpos}

    def parameters(self):
        raise AssertionError("the constructor must validate before it touches the model's tensors")


class _Opt:
    def __init__(self, capture_slots):
        self.capture_slots = capture_slots


def test_constructor_validation_needs_no_device():
    import scattennet_amd as S
    two_pools = _Model([64, 64, 128, 128], 256)
    assert S.BucketedTrainStep(two_pools, _Opt(3), 8, (192, 64, 128), 16).frame_buckets == (64, 128, 192)  # sorted
    with pytest.raises(ValueError, match="bucket 66 is not a multiple of 2\\*\\*n_pool = 4"):
        S.BucketedTrainStep(two_pools, _Opt(2), 8, (64, 66), 16)
    one_pool = _Model([64, 64], 64)
    assert S.BucketedTrainStep(one_pool, _Opt(1), 8, (62,), 16).n_pool == 1
    with pytest.raises(ValueError, match="bucket 63 is not a multiple"):
        S.BucketedTrainStep(one_pool, _Opt(1), 8, (63,), 16)
    with pytest.raises(ValueError, match="bucket 66 exceeds max_position_embeddings = 64"):
        S.BucketedTrainStep(one_pool, _Opt(2), 8, (32, 66), 16)
    with pytest.raises(ValueError, match="capture_slots >= 3"):
        S.BucketedTrainStep(two_pools, _Opt(2), 8, (64, 128, 192), 16)


def test_fused_adam_capture_slots_argument():
    import scattennet_amd as S
    from scattennet_amd import optim
    p = torch.nn.Parameter(torch.zeros(3))
    assert S.FusedAdam([p]).capture_slots == optim.SPARE_TABLES == 2  # the default is unchanged
    assert S.FusedAdam([p], capture_slots=5).capture_slots == 5
    with pytest.raises(ValueError, match="capture_slots"):
        S.FusedAdam([p], capture_slots=-1)
    with pytest.raises(ValueError, match="capture_slots >= 3"):
        S.BucketedTrainStep(_Model([64, 64], 64), S.FusedAdam([p]), 8, (16, 32, 48), 4)


def test_model_counts_its_pooling_stages():
    from scattennet_amd.bucketed import n_pool_of
    for blocks, n in (([64, 64], 1), ([64, 64, 128, 128], 2), ([64], 1), ([64, 64, 128], 2)):
        assert n_pool_of({"residual_blocks": blocks}) == n
    # the same count the model uses for the shift it hands to the kernels
    import scattennet_amd as S
    from tests.golden_util import manifest
    cfg = copy.deepcopy(manifest("manifest_model.json")["fixtures"]["model_small"]["cfg"])
    m = S.MSCA_Net(cfg, list(range(8)))
    assert m.n_pool() == n_pool_of(cfg) == sum(1 for i in range(len(cfg["residual_blocks"])) if i % 2 == 0)


def test_bucket_mode_refuses_torch_compile_tracing(monkeypatch):
    """Out of scope: a clear NotImplementedError, raised before anything touches the device."""
    import scattennet_amd as S
    from scattennet_amd import library
    from tests.golden_util import manifest
    monkeypatch.setattr(torch.compiler, "is_compiling", lambda: True)
    vf = torch.tensor([5], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="valid_frames"):
        library.softmax_rows_apply(torch.zeros(2, 4, 8), valid=(vf, 1))
    cfg = copy.deepcopy(manifest("manifest_model.json")["fixtures"]["model_small"]["cfg"])
    model = S.MSCA_Net(cfg, list(range(8)))
    with pytest.raises(NotImplementedError, match="valid_frames"):
        model(S.pad_batch(_batch(K=16), 8))


def test_new_operator_is_registered_and_the_old_schema_is_unchanged():
    import scattennet_amd  # noqa: F401
    assert str(torch.ops.scatten.softmax_rows.default._schema) == "scatten::softmax_rows(Tensor x) -> Tensor"
    schema = str(torch.ops.scatten.softmax_rows_valid.default._schema)
    assert schema == "scatten::softmax_rows_valid(Tensor x, Tensor valid_frames, SymInt shift) -> Tensor" or \
        schema == "scatten::softmax_rows_valid(Tensor x, Tensor valid_frames, int shift) -> Tensor"
    # the fake implementation: shapes without a device
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        x = torch.empty(2, 5, 16)
        y = torch.ops.scatten.softmax_rows_valid(x, torch.empty(1, dtype=torch.int32), 1)
        assert y.shape == x.shape and y.dtype == x.dtype


class _ModelWithParameter(_Model):
    """For the evaluator and the recognizer, whose constructors take the device from the model."""

    def parameters(self):
        return iter([torch.nn.Parameter(torch.zeros(1))])

    def _students(self):
        return []


def test_a_bad_bucket_is_reported_under_the_callers_own_name():
    import scattennet_amd as S
    m = _ModelWithParameter([64, 64], 64)  # one pooling stage
    with pytest.raises(ValueError, match="^BucketedRecognizer: bucket 33 is not a multiple") as e:
        S.BucketedRecognizer(m, 3, (33,))
    assert "capture_slots" not in str(e.value) and "BucketedTrainStep" not in str(e.value)
    with pytest.raises(ValueError, match="^BucketedEvalStep: bucket 33 is not a multiple") as e:
        S.BucketedEvalStep(m, 3, (33,), 8)
    assert "capture_slots" not in str(e.value) and "BucketedTrainStep" not in str(e.value)
    with pytest.raises(ValueError, match="^BucketedTrainStep: bucket 33 is not a multiple"):
        S.BucketedTrainStep(m, _Opt(1), 3, (33,), 8)
    # neither needs an optimizer, so neither has capture slots to run out of
    rec, bes = S.BucketedRecognizer(m, 3, (16, 32, 48)), S.BucketedEvalStep(m, 3, (16, 32, 48), 8)
    with pytest.raises(ValueError, match="^BucketedTrainStep: 3 buckets need .* capture_slots >= 3"):
        S.BucketedTrainStep(m, _Opt(2), 3, (16, 32, 48), 8)
    for step, name in ((rec, "BucketedRecognizer"), (bes, "BucketedEvalStep")):
        assert step.bucket_for(17) == 32 and not step.captured(32)
        with pytest.raises(ValueError, match=f"^{name}: a batch of 49 frames fits no bucket"):
            step.bucket_for(49)
    with pytest.raises(ValueError, match="^BucketedRecognizer: batch_size must be positive"):
        S.BucketedRecognizer(m, 0, (16,))
    with pytest.raises(ValueError, match="^BucketedEvalStep: batch_size and label_bucket must be positive"):
        S.BucketedEvalStep(m, 3, (16,), 0)


def test_deferred_check_swaps_and_restores():
    from types import SimpleNamespace
    from scattennet_amd.model import deferred_check
    model = SimpleNamespace(check="sync")
    with deferred_check(model):
        assert model.check == "defer"
    assert model.check == "sync"
    model.check = "off"
    with deferred_check(model):
        assert model.check == "off"
    assert model.check == "off"
    model.check = "sync"
    with pytest.raises(KeyError):
        with deferred_check(model):
            assert model.check == "defer"
            raise KeyError("the body failed")
    assert model.check == "sync"


def test_labels_2d_from_both_label_forms():
    from scattennet_amd.heads import labels_2d
    two_d, concat = _batch(), _batch(concat=True)
    assert labels_2d(two_d, 3, "caller") is two_d["gloss_labels"]  # 2-D: as it is
    got = labels_2d(concat, 3, "caller")
    assert got.shape == (3, 3) and got.dtype == two_d["gloss_labels"].dtype
    valid = torch.arange(3)[None, :] < two_d["gloss_lengths"][:, None]
    assert torch.equal(got, two_d["gloss_labels"] * valid)  # the same labels, zero past each clip's length
    with pytest.raises(ValueError, match="^caller: gloss_labels must be .*got \\(3, 3, 1\\)"):
        labels_2d({**two_d, "gloss_labels": two_d["gloss_labels"].unsqueeze(-1)}, 3, "caller")
    with pytest.raises(ValueError, match="^eval_step: gloss_labels must be"):
        labels_2d(two_d, 2, "eval_step")  # (3, S) labels for a batch of two clips
