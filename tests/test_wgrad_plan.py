"""The weight-gradient launch policy (ops._wgrad_plan) is pure Python: which problems share a
launch, and each launch's kernel variant and split-K.  The expected values are what the
scheduler issued before the policy was split from the launcher — recorded from that commit by
running its launcher with `gemm` stubbed, at the default switches and (the *_OFF tables, recorded
the same way) with `_TNR` and / or `_TNB_MIN_K` patched off.  An entry lists the launches in issue
order as (problems, variant, splitk); one tuple of launches where sk_late does not matter, else
{sk_late: launches}."""
import pytest

from scattennet_amd import ops

A, B, C = (256, 256, 2048), (768, 256, 2048), (256, 768, 2048)

DEFAULT = [
    ([A] * 16, {0: [(16, 46, 2)], 3: [(16, 46, 3)]}),
    ([B] * 4, {0: [(4, 46, 4)], 3: [(4, 46, 4)]}),
    ([C] * 4, {0: [(4, 46, 4)], 3: [(4, 46, 4)]}),
    ([A] * 16 + [B] * 4 + [C] * 4, {0: [(16, 46, 2), (4, 46, 4), (4, 46, 4)], 3: [(16, 46, 3), (4, 46, 4), (4, 46, 4)]}),
    ([A] * 12, {0: [(12, 46, 2)], 3: [(12, 46, 3)]}),
    ([A] * 40, {0: [(16, 46, 2), (16, 46, 2), (8, 46, 2)], 3: [(16, 46, 3), (16, 46, 3), (8, 46, 3)]}),
    ([(512, 512, 8192)] * 16, [(16, 43, 1)]),
    ([(1536, 512, 8192)] * 4, [(4, 43, 1)]),
    ([(256, 256, 4096)] * 4, [(4, 43, 1)]),
    ([(256, 256, 4032)] * 4, {0: [(4, 46, 2)], 3: [(4, 46, 3)]}),
    ([(256, 256, 512)] * 4, {0: [(4, 46, 2)], 3: [(4, 46, 2)]}),
    ([(256, 256, 448)] * 4, [(4, 46, 1)]),
    ([(64, 64, 128)] * 2, [(2, 46, 1)]),
    ([(256, 256, 64)] * 4, [(4, 0, 1)]),
    ([(256, 256, 100)] * 8, [(8, 0, 1)]),
    ([(768, 256, 2000)] * 4, [(4, 36, 2)]),
    ([(64, 64, 2000)] * 3, [(3, 0, 7)]),
    ([(64, 32, 300)] * 1, [(1, 0, 1)]),
    ([(128, 128, 1000)] * 1, [(1, 0, 3)]),
    ([(256, 256, 8192)] * 20, [(16, 43, 1), (4, 43, 1)]),
]

TNR_OFF = [  # _TNR False: the LDS-DMA kernels (36 / 0) take variant 46's launches; sk_late never applies
    ([A] * 16, [(16, 36, 2)]),
    ([B] * 4, [(4, 36, 2)]),
    ([C] * 4, [(4, 36, 2)]),
    ([A] * 16 + [B] * 4 + [C] * 4, [(16, 36, 2), (4, 36, 2), (4, 36, 2)]),
    ([A] * 12, [(12, 0, 4)]),
    ([A] * 40, [(16, 36, 2), (16, 36, 2), (8, 0, 6)]),
    ([(512, 512, 8192)] * 16, [(16, 43, 1)]),
    ([(256, 256, 4096)] * 4, [(4, 43, 1)]),
    ([(256, 256, 4032)] * 4, [(4, 0, 8)]),
    ([(256, 256, 512)] * 4, [(4, 0, 2)]),
    ([(256, 256, 448)] * 4, [(4, 0, 1)]),
    ([(64, 64, 128)] * 2, [(2, 0, 1)]),
    ([(768, 256, 2000)] * 4, [(4, 36, 2)]),
    ([(64, 64, 2000)] * 3, [(3, 0, 7)]),
]

TNB_OFF = [  # _TNB_MIN_K 0: variant 46 takes the long reductions too
    ([A] * 16, {0: [(16, 46, 2)], 3: [(16, 46, 3)]}),
    ([B] * 4, {0: [(4, 46, 4)], 3: [(4, 46, 4)]}),
    ([(512, 512, 8192)] * 16, {0: [(16, 46, 2)], 3: [(16, 46, 3)]}),
    ([(1536, 512, 8192)] * 4, {0: [(4, 46, 2)], 3: [(4, 46, 3)]}),
    ([(256, 256, 4096)] * 4, {0: [(4, 46, 2)], 3: [(4, 46, 3)]}),
    ([(256, 256, 8192)] * 20, {0: [(16, 46, 2), (4, 46, 2)], 3: [(16, 46, 3), (4, 46, 3)]}),
    ([(256, 256, 100)] * 8, [(8, 0, 1)]),
]

BOTH_OFF = [
    ([A] * 16, [(16, 36, 2)]),
    ([(512, 512, 8192)] * 16, [(16, 36, 2)]),
    ([(1536, 512, 8192)] * 4, [(4, 36, 1)]),
    ([(256, 256, 4096)] * 4, [(4, 0, 8)]),
    ([(256, 256, 8192)] * 20, [(16, 36, 2), (4, 0, 8)]),
]


def _check(table):
    for keys, want in table:
        for sk_late in (0, 3):
            exp = want[sk_late] if isinstance(want, dict) else want
            plan = ops._wgrad_plan(keys, sk_late)
            assert [(len(ix), v, sk) for ix, v, sk in plan] == exp, (keys[0], len(keys), sk_late)
            # every problem is launched exactly once, with problems of its own shape only
            assert sorted(i for ix, _, _ in plan for i in ix) == list(range(len(keys)))
            assert all(len({keys[i] for i in ix}) == 1 for ix, _, _ in plan)
        assert ops._wgrad_plan(keys) == ops._wgrad_plan(keys, 0)


def test_default_switches():
    _check(DEFAULT)


def test_variant_46_switched_off(monkeypatch):
    monkeypatch.setattr(ops, "_TNR", False)
    _check(TNR_OFF)


def test_tile_43_switched_off(monkeypatch):
    monkeypatch.setattr(ops, "_TNB_MIN_K", 0)
    _check(TNB_OFF)


def test_both_switched_off(monkeypatch):
    monkeypatch.setattr(ops, "_TNR", False)
    monkeypatch.setattr(ops, "_TNB_MIN_K", 0)
    _check(BOTH_OFF)


@pytest.mark.parametrize("sk_late,sk_a", [(0, 2), (3, 3)])
def test_indices_map_each_problem_to_its_launch(sk_late, sk_a):
    keys = [A] * 16 + [B] * 4 + [C] * 4
    assert ops._wgrad_plan(keys, sk_late) == [(list(range(16)), 46, sk_a), (list(range(16, 20)), 46, 4),
                                              (list(range(20, 24)), 46, 4)]
    # interleaved shapes: launches in order of each shape's first problem, indices by shape
    # (too few tiles here for the FFN shapes' split 4)
    keys = [A, B, A, C, B, A]
    assert ops._wgrad_plan(keys, sk_late) == [([0, 2, 5], 46, sk_a), ([1, 4], 46, sk_a), ([3], 46, sk_a)]


def test_an_empty_section_launches_nothing():
    assert ops._wgrad_plan([]) == []


def test_the_plan_needs_no_gpu_library(monkeypatch):
    """Policy only: the plan is made without loading the HIP library."""
    def no_lib():
        raise AssertionError("_wgrad_plan loaded the library")
    monkeypatch.setattr(ops.L, "lib", no_lib)
    assert ops._wgrad_plan([A] * 3) == [([0, 1, 2], 46, 2)]
