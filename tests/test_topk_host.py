"""Top-K recommendation, the parts that need no GPU: the three launchers are declared, bound and exported, and torch.ops.ader.topk_items
traces under FakeTensorMode with the documented shapes and dtypes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ader_topk_kmax", "ader_topk_ranges", "ader_topk_items")


@pytest.fixture(scope="module")
def lib_path():
    from ader_amd import build
    return build.build()


def test_launchers_are_declared_bound_and_exported(lib_path):
    import ctypes

    import torch  # noqa: F401  (one HIP runtime for the process, see ader_amd/_lib.py)
    from ader_amd import _lib
    header = open(os.path.join(ROOT, "include", "ader_hip.h")).read()
    lib = ctypes.CDLL(lib_path)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert n in _lib.exported_symbols() and hasattr(lib, n), n
    assert lib.ader_topk_kmax() == 64
    # a multiple of 8 (the block -> (range, chunk) mapping); about one workgroup per CU: never more than 256 over the chunks
    for N, Bp in ((1, 64), (650, 128), (40000, 128), (1_000_000, 1024), (1_000_000, 64), (25750, 192)):
        r = lib.ader_topk_ranges(N, Bp)
        tiles = (N + 63) // 64
        assert r % 8 == 0 and r >= 8, (N, Bp, r)
        assert r == 8 or (r * (Bp // 64) <= 256 and r <= (tiles + 7) // 8 * 8), (N, Bp, r)
    assert lib.ader_topk_ranges(650, 128) >= 11 and lib.ader_topk_ranges(40000, 128) < 625


def test_topk_items_traces_under_fake_tensors(lib_path):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb = torch.empty(5, 150), torch.empty(101, 150)
        items, scores = torch.ops.ader.topk_items(rep, emb, None, 100, 20)
        assert tuple(items.shape) == (5, 20) and items.dtype == torch.int32
        assert tuple(scores.shape) == (5, 20) and scores.dtype == torch.float32
        seen = torch.empty(5, 50, dtype=torch.int32)
        items, scores = torch.ops.ader.topk_items(rep, emb, seen, 100, 64)
        assert tuple(items.shape) == (5, 64) and tuple(scores.shape) == (5, 64)
