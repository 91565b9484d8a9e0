"""Host side of the x3 top-K recommendation (no GPU): the exports, the options, the fake-tensor trace of the operator, and the two
properties the kernels rest on, emulated on the CPU: (1) the kept set C = {n : !(s3_n < t3 - d)} of every catalog prefix contains the
float32-chain top-k, and the best k of the final C by the exact key are the stable argsort head; (2) on Gaussian operands the band
below the k-th best score holds at most half the default `band` items, per item range and over the catalog -- the condition under
which tests/test_gpu_topk_x3.py asserts "no overflow"."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ader_topk_x3_kmax", "ader_topk_x3_ranges", "ader_topk_items_x3")
NORM_UP = 1.0005            # RANK_NORM_UP of csrc/logits_x3.hip


@pytest.fixture(scope="module")
def lib(request):
    import ctypes

    from ader_amd import build
    import torch  # noqa: F401  (one HIP runtime for the process, see ader_amd/_lib.py)
    return ctypes.CDLL(build.build())


def test_launchers_are_declared_bound_and_exported(lib):
    from ader_amd import _lib
    header = open(os.path.join(ROOT, "include", "ader_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert n in _lib.exported_symbols() and hasattr(lib, n), n
    kmax = lib.ader_topk_x3_kmax()
    assert 20 <= kmax <= 64
    # a multiple of 8 (the block -> (range, chunk) mapping); about one workgroup per CU: never more than 256 over the 128-row chunks
    for N, Bp in ((1, 128), (650, 128), (40000, 128), (1_000_000, 1024), (1_000_000, 128), (25750, 256)):
        r = lib.ader_topk_x3_ranges(N, Bp)
        blocks = (N + 31) // 32
        assert r % 8 == 0 and r >= 8, (N, Bp, r)
        assert r == 8 or (r * (Bp // 128) <= 256 and r <= (blocks + 7) // 8 * 8), (N, Bp, r)
    assert lib.ader_topk_x3_ranges(40000, 128) < 1250          # a workgroup walks several blocks


def test_options_and_defaults():
    from ader_amd.engine import Engine, infer
    from ader_amd.main import _BUILD_FLAGS, build_parser
    from ader_amd.model import Ader
    flag = [f for f in _BUILD_FLAGS if f[0] == "topk_dtype"]
    assert len(flag) == 1 and flag[0][1] == "f32" and flag[0][3] == ("f32", "x3")
    assert build_parser().parse_args([]).topk_dtype == "f32"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--topk_dtype", "bf16"])
    assert inspect.signature(Engine.__init__).parameters["topk_dtype"].default == "f32"
    rc = inspect.signature(Engine.recommend).parameters
    assert list(rc)[1:] == ["seq", "k", "max_item", "exclude_seen", "dtype", "band"]
    assert rc["dtype"].default is None and rc["band"].default is None and rc["exclude_seen"].default is False
    assert inspect.signature(Ader.recommend).parameters["dtype"].default is None
    assert infer.TOPK_DTYPES == ("f32", "x3") and infer.TOPK_X3_BAND == 16
    assert Engine.last_topk_stats is None
    with pytest.raises(RuntimeError, match="topk_dtype"):        # validated before anything touches the GPU
        Engine(100, topk_dtype="bf16")


def test_topk_items_x3_traces_under_fake_tensors(lib):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb = torch.empty(5, 150), torch.empty(101, 150)
        items, scores = torch.ops.ader.topk_items_x3(rep, emb, None, 100, 20)
        assert tuple(items.shape) == (5, 20) and items.dtype == torch.int32
        assert tuple(scores.shape) == (5, 20) and scores.dtype == torch.float32
        seen = torch.empty(5, 50, dtype=torch.int32)
        items, scores = torch.ops.ader.topk_items_x3(rep, emb, seen, 100, 33)
        assert tuple(items.shape) == (5, 33) and tuple(scores.shape) == (5, 33)


# ---------------------------------------------------------------------------------------------- the x3 emulation (tests/test_rank_x3_host.py's)
def _split(x):
    """hi = bf16(x), lo = bf16(x - hi), round-to-nearest-even, as k_lx3_prep and the block staging cut their operands (numpy float32)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi.numpy(), lo.numpy()


def _s3_pairs(r, e):
    """x3 score of r [B,H] against e [B,m,H] (row b with its own m table rows) or [m,H] (shared): three terms per k (lo.hi, hi.lo, hi.hi,
    the kernel's order; products of two bf16 values are exact in float32), accumulated in float32 in k order -> float32 [B,m]."""
    rh, rl = _split(r)
    eh, el = _split(e)
    if e.ndim == 2:
        eh, el = eh[None], el[None]
    s = np.zeros((r.shape[0], eh.shape[1]), dtype=np.float32)
    for k in range(r.shape[1]):
        s = s + el[:, :, k] * rh[:, None, k]
        s = s + eh[:, :, k] * rl[:, None, k]
        s = s + eh[:, :, k] * rh[:, None, k]
    assert s.dtype == np.float32
    return s


def _s32(r, e):
    """The float32 chain of the exact kernels: one fma per k, in k order (r [B,H], e [N,H] -> float32 [B,N])."""
    s = np.zeros((r.shape[0], e.shape[0]), dtype=np.float32)
    for k in range(r.shape[1]):
        s = (s.astype(np.float64) + e[None, :, k].astype(np.float64) * r[:, None, k].astype(np.float64)).astype(np.float32)
    return s


def _delta(r, e):
    """k_rank_delta's band width d_b = KAPPA |rep_b| Emax, both norms rounded up, in float32."""
    from ader_amd.engine.infer import RANK_X3_KAPPA
    emax = np.float32(np.sqrt((e.astype(np.float64) ** 2).sum(1)).max() * NORM_UP)
    rn = (np.sqrt((r.astype(np.float64) ** 2).sum(1)) * NORM_UP).astype(np.float32)
    return (np.float32(RANK_X3_KAPPA) * rn * emax).astype(np.float32)


def _exact_order(s):
    """Item indices of one row by the exact key: score descending, id ascending."""
    return np.argsort(-s, kind="stable")


def _operands(kind, H, rs):
    """tests/test_rank_x3_host.py's operands, restated."""
    B, N = 24, 96
    if kind == "random":
        r = rs.standard_normal((B, H)) * np.exp(rs.uniform(-3, 3, size=(B, 1)))
        e = rs.standard_normal((N, H)) * np.exp(rs.uniform(-3, 3, size=(N, 1)))
    else:
        base = 1.0 + 2.0 ** -8 + 2.0 ** -16 + rs.randint(1, 128, size=(B + N, H)) * 2.0 ** -23
        x = base * 2.0 ** rs.randint(-1, 1, size=(B + N, 1))
        r, e = x[:B], x[B:]
    return r.astype(np.float32), e.astype(np.float32)


def _plant_near_ties(r, e, k, rs):
    """Copies of the k-th best item of row 0 at other ids, one channel moved by 1..4 ulp: near-ties across the k boundary."""
    e = e.copy()
    kth = _exact_order(_s32(r[:1], e)[0])[k - 1]
    others = [n for n in rs.permutation(e.shape[0]) if n != kth][:6]
    for j, n in enumerate(others):
        e[n] = e[kth]
        c = int(np.argmax(np.abs(e[n])))
        e[n, c] = np.float32(e[n, c]) + np.float32((j % 4 + 1) * (1 if j & 1 else -1)) * np.spacing(np.float32(e[n, c]))
    return e


def _check_superset(r, e, k):
    s3, s = _s3_pairs(r, e), _s32(r, e)
    d = _delta(r, e)
    N = e.shape[0]
    for b in range(r.shape[0]):
        for end in sorted(set(list(range(32, N, 32)) + [N])):
            if end < k:
                continue
            t3 = np.sort(s3[b, :end])[end - k]                   # the k-th largest x3 score of the prefix
            lo = np.float32(t3 - d[b])
            C = np.nonzero(~(s3[b, :end] < lo))[0]
            top = _exact_order(s[b, :end])[:k]
            assert set(top.tolist()) <= set(C.tolist()), (b, end)
            if end == N:
                best = C[_exact_order(s[b, C])[:k]]              # (C ascending: a stable sort of it keeps the id order among ties)
                assert np.array_equal(best, _exact_order(s[b])[:k]), b


@pytest.mark.parametrize("H", [12, 64, 150])
@pytest.mark.parametrize("kind", ["random", "adversarial", "near_ties"])
def test_kept_set_contains_the_float32_chain_topk(kind, H):
    rs = np.random.RandomState(H + len(kind))
    r, e = _operands("random" if kind == "near_ties" else kind, H, rs)
    for k in (5, 20):
        _check_superset(r, _plant_near_ties(r, e, k, rs) if kind == "near_ties" else e, k)


# ---------------------------------------------------------------------------------------------- band populations of Gaussian operands
# B, N, H, seed, scale, ks: the Gaussian operands of tests/test_gpu_topk_x3.py (rep drawn first, then the table)
GAUSS = [(130, 777, 150, 5, 0.05, (20, 64)), (70, 40000, 150, 7, 0.05, (20, 64)), (130, 4097, 12, 9, 1.0, (20,)),
         (257, 100000, 64, 3, 0.05, (20,))]
MARGIN = 32                 # candidates beyond k that get the x3 emulation


def _band_population(r, e, s64, d, k):
    """Per row: #{n : !(s3_n < t3 - d)} - k over the items of e (t3 = the k-th largest x3 score), 0 where there are no more than k items.
    The x3 emulation runs on the k + MARGIN best items by float64 score only: with |s3 - s64| <= d/2 (asserted on them, derived in
    csrc/logits_x3.hip) an item more than 3 d below the float64 k-th best is below t3 - d, so the rest cannot be in the band -- asserted
    on the best item left out."""
    B, n = s64.shape
    if n <= k:
        return np.zeros(B, dtype=np.int64)
    m = min(n, k + MARGIN)
    head = np.argpartition(-s64, m, axis=1)[:, :m + 1] if m < n else np.tile(np.arange(n), (B, 1))
    order = np.take_along_axis(head, np.argsort(-np.take_along_axis(s64, head, axis=1), axis=1, kind="stable"), axis=1)
    kth = np.take_along_axis(s64, order[:, k - 1:k], axis=1)[:, 0]
    if m < n:
        left_out = np.take_along_axis(s64, order[:, m:m + 1], axis=1)[:, 0]
        assert (left_out < kth - 3.0 * d).all()
    idx = order[:, :m]
    s3 = _s3_pairs(r, e[idx])
    assert (np.abs(s3.astype(np.float64) - np.take_along_axis(s64, idx, axis=1)) <= 0.5 * d[:, None]).all()
    t3 = np.sort(s3, axis=1)[:, m - k]
    lo = (t3 - d).astype(np.float32)
    return (~(s3 < lo[:, None])).sum(1) - k


@pytest.mark.parametrize("case", range(len(GAUSS)))
def test_gaussian_band_populations_stay_under_half_the_band(lib, case):
    from ader_amd.engine.infer import TOPK_X3_BAND
    B, N, H, seed, scale, ks = GAUSS[case]
    rs = np.random.RandomState(seed)
    r = rs.standard_normal((B, H)).astype(np.float32)
    emb = (rs.standard_normal((N + 1, H)) * scale).astype(np.float32)
    e = emb[1:]
    d = _delta(r, e).astype(np.float64)
    s64 = r.astype(np.float64) @ e.astype(np.float64).T
    ranges = lib.ader_topk_x3_ranges(N, (min(B, 1024) + 127) // 128 * 128)
    per = ((N + 31) // 32 + ranges - 1) // ranges * 32                 # items per range: k_lx3t's partition
    for k in sorted(set(ks) | {lib.ader_topk_x3_kmax()}):
        worst_g = int(_band_population(r, e, s64, d, k).max())
        worst_r = max(int(_band_population(r, e[a:a + per], s64[:, a:a + per], d, k).max()) for a in range(0, N, per))
        print("B=%d N=%d H=%d k=%d: worst band population per range %d, global %d" % (B, N, H, k, worst_r, worst_g))
        assert worst_r <= TOPK_X3_BAND // 2 and worst_g <= TOPK_X3_BAND // 2
