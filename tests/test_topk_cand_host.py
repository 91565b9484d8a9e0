"""candidate_ids (ader_amd/engine/infer.py): the host normalisation of Engine.recommend's candidate list into the form
ader_topk_items_cand takes -- sorted, unique int32 ids <= N; anything that is not a 1-D list of item ids raises.  No GPU."""
import numpy as np
import pytest
import torch

from ader_amd.engine.infer import candidate_ids


def test_unsorted_input_with_duplicates_becomes_sorted_unique_int32():
    out = candidate_ids(np.array([9, 3, 3, 7, 1, 9, 2], dtype=np.int64), 10, 10)
    assert isinstance(out, np.ndarray) and out.dtype == np.int32 and out.ndim == 1 and out.flags["C_CONTIGUOUS"]
    assert out.tolist() == [1, 2, 3, 7, 9]
    assert np.all(np.diff(out) > 0)


def test_ids_above_n_up_to_item_num_are_dropped():
    out = candidate_ids([5, 11, 10, 20, 1], 10, 20)
    assert out.tolist() == [1, 5, 10]
    assert candidate_ids([11, 20], 10, 20).tolist() == []
    assert candidate_ids([11, 20], 10, 20).dtype == np.int32


@pytest.mark.parametrize("bad", [0, -4, 21])
def test_an_id_outside_1_to_item_num_raises(bad):
    with pytest.raises(RuntimeError):
        candidate_ids([3, bad, 5], 10, 20)
    with pytest.raises(RuntimeError):
        candidate_ids(torch.tensor([3, bad, 5]), 10, 20)


@pytest.mark.parametrize("bad", [np.array([1.0, 2.0]), np.array([[1, 2], [3, 4]]), np.array([True, False, True]),
                                 np.array(3), np.zeros(0, dtype=np.float32)])
def test_a_float_a_2d_a_bool_and_a_0d_array_raise(bad):
    with pytest.raises(RuntimeError):
        candidate_ids(bad, 10, 20)
    with pytest.raises(RuntimeError):
        candidate_ids(torch.from_numpy(np.asarray(bad)), 10, 20)


def test_an_empty_list_stays_empty():
    for empty in ([], (), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64), torch.zeros(0, dtype=torch.int64)):
        out = candidate_ids(empty, 10, 20)
        assert out.dtype == np.int32 and out.shape == (0,)


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64, np.uint8])
def test_numpy_and_torch_inputs_agree(dtype):
    rs = np.random.RandomState(0)
    a = rs.randint(1, 101, size=400).astype(dtype)
    ref = candidate_ids(a, 80, 100)
    assert ref.tolist() == sorted({int(x) for x in a if x <= 80})
    got = candidate_ids(torch.from_numpy(a), 80, 100)
    assert got.dtype == ref.dtype and np.array_equal(got, ref)
    assert np.array_equal(candidate_ids(a.tolist(), 80, 100), ref)
    assert np.array_equal(candidate_ids(ref, 80, 100), ref)          # idempotent


@pytest.fixture(scope="module")
def lib():
    import ctypes

    from ader_amd import build
    return ctypes.CDLL(build.build())


def test_launcher_is_declared_bound_and_exported(lib):
    import os
    import re

    from ader_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ader_hip.h")).read()
    assert re.search(r"\bint\s+ader_topk_items_cand\s*\(", header)
    assert "ader_topk_items_cand" in _lib.exported_symbols() and hasattr(lib, "ader_topk_items_cand")
    assert len(_lib._SIGS["ader_topk_items_cand"]) == 17
    assert lib.ader_topk_ranges(0, 64) == 8            # an empty list: eight empty ranges, every row padding


def test_topk_items_cand_traces_under_fake_tensors(lib):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb, cand = torch.empty(5, 150), torch.empty(101, 150), torch.empty(40, dtype=torch.int32)
        items, scores = torch.ops.ader.topk_items_cand(rep, emb, cand, None, 100, 20)
        assert tuple(items.shape) == (5, 20) and items.dtype == torch.int32
        assert tuple(scores.shape) == (5, 20) and scores.dtype == torch.float32
        seen = torch.empty(5, 50, dtype=torch.int32)
        items, scores = torch.ops.ader.topk_items_cand(rep, emb, cand, seen, 100, 33)
        assert tuple(items.shape) == (5, 33) and tuple(scores.shape) == (5, 33)


def test_the_candidate_call_is_a_method_of_its_own_and_recommend_keeps_its_parameters():
    import inspect

    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    ra = inspect.signature(Engine.recommend_among).parameters
    assert list(ra)[1:] == ["seq", "k", "candidates", "max_item", "exclude_seen", "dtype"]
    assert ra["max_item"].default is None and ra["exclude_seen"].default is False and ra["dtype"].default is None
    assert "candidates" not in inspect.signature(Engine.recommend).parameters
    assert inspect.signature(Ader.recommend).parameters["candidates"].default is None
