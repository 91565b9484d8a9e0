"""Wide top-K (csrc/topk.hip, Engine.recommend_wide) without a GPU: the exports, the slab schedule ader_topk_wide_slabs as a pure
host function, and a numpy emulation of slab-and-select on the library's own slab boundaries -- per row a list of 64-bit keys, every
key of a slab that beats the row's threshold appended, the list cut to its best k after the slab -- against the head of the stable
argsort.  The emulation also backs the premise of tests/test_gpu_topk_wide.py: on Gaussian operands at its shapes no list outgrows cap,
so the unflagged path alone can meet what those tests assert."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

GROWTH = 32     # the slab rule's constant (csrc/topk.hip: WIDE_GROWTH; DESIGN.md says how it was chosen)
NAMES = ("ader_topk_wide_kmax", "ader_topk_wide_cap", "ader_topk_wide_slabs", "ader_topk_items_wide")
# the shapes of tests/test_gpu_topk_wide.py: item_num, T, H, L, heads, B, N, k, cap (None: the default)
GPU_SHAPES = [(700, 50, 150, 2, 1, 70, 650, 100, 256),
              (1000, 50, 150, 2, 3, 130, 777, 65, 192),
              (5000, 20, 150, 1, 1, 65, 4097, 1024, 4096),
              (64, 8, 12, 1, 1, 3, 33, 100, 192),
              (2000, 20, 150, 1, 1, 1030, 1999, 70, None),
              (40000, 20, 150, 1, 1, 70, 40000, 300, 1024),
              (20000, 20, 150, 1, 1, 260, 20000, 64, None)]


@pytest.fixture(scope="module")
def lib():
    from ader_amd import build
    lb = ctypes.CDLL(build.build())
    lb.ader_topk_wide_slabs.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return lb


def slabs(lib, N, k, cap):
    """The library's slab boundaries [0, ..., N] as a list."""
    n = lib.ader_topk_wide_slabs(N, k, cap, None, 0)
    assert n >= 1
    out = np.full(n + 3, -7, dtype=np.int32)
    assert lib.ader_topk_wide_slabs(N, k, cap, out.ctypes.data, n + 1) == n
    assert (out[n + 1:] == -7).all()                     # nothing beyond max ints is written
    return out[:n + 1].tolist()


def test_exports_and_limits(lib):
    from ader_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ader_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
    assert len(_lib._SIGS["ader_topk_items_wide"]) == 19 and len(_lib._SIGS["ader_topk_wide_slabs"]) == 5
    assert lib.ader_topk_wide_kmax() == 1024 and lib.ader_topk_wide_cap() == 4096
    assert lib.ader_topk_kmax() == 64                    # the narrow path keeps its limit


@pytest.mark.parametrize("N,k,cap", [(1, 1, 128), (33, 100, 192), (650, 100, 256), (650, 65, 192), (777, 65, 192), (4097, 300, 1024),
                                     (4097, 1024, 4096), (1999, 70, 4096), (8300, 100, 256), (40000, 300, 1024), (40000, 1024, 4096),
                                     (200000, 1024, 4096), (200000, 100, 4096), (1_000_000, 64, 4096), (1_000_000, 1024, 1088),
                                     (4096, 1, 4096), (4160, 1, 4096)])
def test_slab_schedule_obeys_the_rule(lib, N, k, cap):
    b = slabs(lib, N, k, cap)
    assert b[0] == 0 and b[-1] == N and all(y > x for x, y in zip(b, b[1:]))
    assert all(x % 64 == 0 for x in b[:-1])
    assert b[1] == min(N, cap)
    for seen, nxt in zip(b[1:], b[2:]):
        # max(64, 64 floor(seen min(1, (cap - k) / (GROWTH k)) / 64)) in integers: floor(floor(x) / 64) == floor(x / 64)
        rule = max(64, 64 * ((seen * min(cap - k, GROWTH * k)) // (GROWTH * k * 64)))
        assert nxt - seen == min(rule, N - seen), (seen, nxt)
    if cap - k >= GROWTH * k:
        assert all(nxt - seen == min(seen, N - seen) for seen, nxt in zip(b[1:], b[2:]))      # growth capped at doubling


def test_slab_schedule_rejects_bad_arguments(lib):
    f = lib.ader_topk_wide_slabs
    assert f(1000, 100, 256, None, 0) > 0
    for k in (0, -1, 1025):
        assert f(1000, k, 4096, None, 0) == -2
    for k, cap in ((100, 163), (100, 128), (100, 200), (100, 4160), (1024, 1024), (1, 0), (1, 64), (1, 64 + 63)):
        assert f(1000, k, cap, None, 0) == -2, (k, cap)
    assert f(0, 100, 256, None, 0) == -2
    assert f(1000, 1, 64 + 64, None, 0) > 0 and f(1000, 1024, 1088, None, 0) > 0 and f(1000, 1024, 4096, None, 0) > 0


# ------------------------------------------------------------------------------------------------ emulation of slab and select
def keys_of(scores):
    """topk_key (csrc/topk_key.h) of a float32 row over items 1..N: order-preserving score bits above, the complemented id below."""
    u = (np.asarray(scores, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    u = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    ids = np.arange(1, len(u) + 1, dtype=np.uint32)
    return (u.astype(np.uint64) << np.uint64(32)) | (~ids).astype(np.uint64)


def emulate(scores, seen, bounds, k, cap):
    """Slab and select in numpy -> (items int32 [n,k], scores float32 [n,k], largest list after slab 0, overflowed rows)."""
    n, N = scores.shape
    items, out = np.zeros((n, k), dtype=np.int32), np.full((n, k), -np.inf, dtype=np.float32)
    max_list, overflowed = 0, 0
    for b in range(n):
        key = keys_of(scores[b])
        ok = np.ones(N, dtype=bool)
        if seen is not None:
            s = seen[b][(seen[b] > 0) & (seen[b] <= N)]
            ok[s - 1] = False
        lst, thr, over = np.zeros(0, dtype=np.uint64), np.uint64(0), False
        for j, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
            c = key[lo:hi][ok[lo:hi]]
            c = c[c > thr]
            total = len(lst) + len(c)
            if j > 0:
                max_list = max(max_list, total)
            over |= total > cap
            lst = np.sort(np.concatenate([lst, c]))[::-1][:k]
            thr = lst[k - 1] if len(lst) >= k else np.uint64(0)
        overflowed += bool(over)
        m = len(lst)
        items[b, :m] = (~(lst & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int32)
        hi32 = (lst >> np.uint64(32)).astype(np.uint32)
        out[b, :m] = np.where(hi32 & np.uint32(0x80000000), hi32 ^ np.uint32(0x80000000), ~hi32).view(np.float32)
    return items, out, max_list, overflowed


def reference(lg, seen, k):
    """The contract: the head of the stable argsort of -lg, seen columns at -inf, item 0 / -inf padding."""
    lg = np.array(lg, dtype=np.float32)
    n, N = lg.shape
    if seen is not None:
        for b in range(n):
            s = seen[b][(seen[b] > 0) & (seen[b] <= N)]
            lg[b, s - 1] = -np.inf
    order = np.argsort(-lg, axis=1, kind="stable")
    m = min(k, N)
    items, scores = np.zeros((n, k), dtype=np.int32), np.full((n, k), -np.inf, dtype=np.float32)
    sc = np.take_along_axis(lg, order[:, :m], axis=1)
    it = (order[:, :m] + 1).astype(np.int32)
    it[sc == -np.inf] = 0
    items[:, :m], scores[:, :m] = it, sc
    return items, scores


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("N,k,cap", [(33, 100, 192), (650, 100, 256), (650, 65, 192), (700, 640, 704), (1500, 1, 64 + 64),
                                     (4097, 300, 1024), (300, 300, 384), (257, 256, 320)])
def test_emulation_on_tie_heavy_integer_scores_equals_the_stable_argsort_head(lib, N, k, cap, exclude):
    rs = np.random.RandomState(N + k)
    n = 6
    lg = rs.randint(-3, 4, size=(n, N)).astype(np.float32)            # seven values: every place is inside a tie
    lg[1] = 0.0
    lg[2] = np.sort(lg[2])[::-1]
    lg[3, ::2] = -0.0
    seen = rs.randint(0, N + 40, size=(n, 23)).astype(np.int32) if exclude else None
    items, scores, max_list, overflowed = emulate(lg, seen, slabs(lib, N, k, cap), k, cap)
    ri, rsc = reference(lg, seen, k)
    assert overflowed == 0 and max_list <= cap           # a later item loses every tie: ties only keep keys out of the list
    assert np.array_equal(items, ri)
    assert np.array_equal(scores, rsc)                   # (by value: the key folds -0 onto +0, as == does)


@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_gaussian_operands_keep_every_list_within_cap_at_the_gpu_shapes(lib, shape):
    """The premise of the GPU contract tests: they assert overflowed_rows == 0 and max_list <= cap, which the kernels can only meet if
    the schedule leaves room -- here with numpy float32 logits of Gaussian operands (not the MFMA chain: the list lengths depend on the
    order statistics, not on the last bit)."""
    item_num, T, H, L, heads, B, N, k, cap = shape
    cap = lib.ader_topk_wide_cap() if cap is None else cap
    rs = np.random.RandomState(17)
    rep = rs.standard_normal((min(B, 130), H)).astype(np.float32)
    emb = (rs.standard_normal((N, H)) * 0.05).astype(np.float32)
    lg = rep @ emb.T
    bounds = slabs(lib, N, k, cap)
    items, scores, max_list, overflowed = emulate(lg, None, bounds, k, cap)
    assert overflowed == 0 and max_list <= cap, (max_list, cap)
    if len(bounds) > 2:
        assert max_list >= min(k, N)
    ri, rsc = reference(lg, None, k)
    assert np.array_equal(items, ri) and np.array_equal(scores.view(np.int32), rsc.view(np.int32))


def test_ascending_scores_overflow_the_list(lib):
    """What the overflow tests of tests/test_gpu_topk_wide.py rely on: with scores ascending in the item id every item passes every
    threshold, and at N = 8300, k = 100, cap = 256 some slab is larger than the free room cap - k."""
    b = slabs(lib, 8300, 100, 256)
    assert max(y - x for x, y in zip(b[1:], b[2:])) > 256 - 100
    lg = np.arange(8300, dtype=np.float32)[None, :] * np.float32(0.25)
    _, _, max_list, overflowed = emulate(lg, None, b, 100, 256)
    assert overflowed == 1 and max_list > 256


def test_recommend_wide_parameter_list():
    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    p = inspect.signature(Engine.recommend_wide).parameters
    assert list(p)[1:] == ["seq", "k", "max_item", "exclude_seen", "cap"]
    assert p["max_item"].default is None and p["exclude_seen"].default is False and p["cap"].default is None
    r = inspect.signature(Engine.recommend).parameters                 # the narrow calls keep theirs
    assert list(r)[1:] == ["seq", "k", "max_item", "exclude_seen", "dtype", "band"]
    assert list(inspect.signature(Engine.recommend_among).parameters)[1:] == ["seq", "k", "candidates", "max_item", "exclude_seen", "dtype"]
    assert list(inspect.signature(Ader.recommend).parameters)[1:] == ["seq", "k", "max_item", "exclude_seen", "dtype", "candidates"]


def test_topk_items_wide_traces_under_fake_tensors(lib):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb = torch.empty(5, 150), torch.empty(1001, 150)
        items, scores, over = torch.ops.ader.topk_items_wide(rep, emb, None, 1000, 300, 1024)
        assert tuple(items.shape) == (5, 300) and items.dtype == torch.int32
        assert tuple(scores.shape) == (5, 300) and scores.dtype == torch.float32
        assert tuple(over.shape) == (5,) and over.dtype == torch.int32
        seen = torch.empty(5, 50, dtype=torch.int32)
        items, scores, over = torch.ops.ader.topk_items_wide(rep, emb, seen, 1000, 65, 4096)
        assert tuple(items.shape) == (5, 65) and tuple(scores.shape) == (5, 65)
