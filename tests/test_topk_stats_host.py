"""Top-K with model probabilities (csrc/topk_stats.hip, Engine.row_stats / recommend_stats, Ader.recommend_probs) without a GPU: the
call surface, the validation that precedes every device call, log_probs / probs, the exports, and a numpy float32 emulation of the
kernels' accumulate and merge (csrc/row_stats.h): the float32 state (m, l, u) = (max, sum exp(s - m), sum exp(s - m) (s - m)) per lane;
the lanes of a range, then the ranges of a row, moved to their common maximum and added in a fixed order in double; lse = m + log l,
entropy = log l - u / l, rounded once."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

F = np.float32
NAMES = ("ader_row_stats_floats", "ader_row_stats", "ader_topk_items_stats")
CAP = 64 * 2.0 ** -24      # the issue's cap on the GPU tolerance: 4 ulp at lse in [8, 16)


@pytest.fixture(scope="module")
def lib():
    from ader_amd import build
    lb = ctypes.CDLL(build.build())
    return lb


# ------------------------------------------------------------------------------------------------ call surface
def test_signatures_and_defaults():
    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    p = inspect.signature(Engine.row_stats).parameters
    assert list(p)[1:] == ["seq", "max_item"] and p["max_item"].default is None
    p = inspect.signature(Engine.recommend_stats).parameters
    assert list(p)[1:] == ["seq", "k", "max_item", "exclude_seen"]
    assert p["max_item"].default is None and p["exclude_seen"].default is False
    p = inspect.signature(Ader.row_stats).parameters
    assert list(p)[1:] == ["seq", "max_item"] and p["max_item"].default is None
    p = inspect.signature(Ader.recommend_probs).parameters
    assert list(p)[1:] == ["seq", "k", "max_item", "exclude_seen", "candidates", "form"]
    assert p["max_item"].default is None and p["exclude_seen"].default is False and p["candidates"].default is None
    assert p["form"].default == "prob"


def test_the_existing_parameter_lists_are_unchanged():
    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    assert list(inspect.signature(Engine.recommend).parameters)[1:] == ["seq", "k", "max_item", "exclude_seen", "dtype", "band"]
    assert list(inspect.signature(Ader.recommend).parameters)[1:] == ["seq", "k", "max_item", "exclude_seen", "dtype", "candidates"]


def _engine_without_device():
    """An engine that holds a catalog size and nothing else: any step past the argument checks raises AttributeError."""
    from ader_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.item_num = 100
    return eng


def test_arguments_are_checked_before_any_device_call(lib):
    from ader_amd.model import Ader
    eng = _engine_without_device()
    seq = np.ones((2, 5), dtype=np.int32)
    kmax = lib.ader_topk_kmax()
    for bad_k in (0, -1, kmax + 1):
        with pytest.raises(RuntimeError, match="recommend_stats: k"):
            eng.recommend_stats(seq, bad_k)
    for bad_n in (0, 101, -3):
        with pytest.raises(RuntimeError, match="recommend_stats: max_item"):
            eng.recommend_stats(seq, 5, bad_n)
        with pytest.raises(RuntimeError, match="row_stats: max_item"):
            eng.row_stats(seq, bad_n)
    with pytest.raises(AttributeError):                   # valid arguments go on to the device state, which this engine lacks
        eng.row_stats(seq, 50)
    model = Ader.__new__(Ader)
    model.engine = eng
    for bad_form in ("probs", "logit", None, 1):
        with pytest.raises(RuntimeError, match="form"):
            model.recommend_probs(seq, 5, form=bad_form)
    with pytest.raises(RuntimeError, match="recommend_stats: k"):
        model.recommend_probs(seq, 0)
    with pytest.raises(RuntimeError, match="recommend_stats: max_item"):
        model.recommend_probs(seq, 5, max_item=101)


def test_log_probs_and_probs_with_padding():
    from ader_amd.engine.infer import log_probs, probs
    scores = np.array([[2.5, 1.0, -np.inf], [0.25, -np.inf, -np.inf]], dtype=F)
    lse = np.array([3.0, 0.25], dtype=F)
    lp, p = log_probs(scores, lse), probs(scores, lse)
    assert lp.dtype == F and p.dtype == F and lp.shape == p.shape == scores.shape
    assert np.array_equal(lp.view(np.int32), (scores - lse[:, None]).view(np.int32))
    assert np.isneginf(lp[0, 2]) and np.isneginf(lp[1, 1:]).all()
    assert (p[0, 2] == 0.0) and (p[1, 1:] == 0.0).all() and p[1, 0] == 1.0
    assert np.array_equal(p.view(np.int32), np.exp((scores - lse[:, None]).astype(F)).view(np.int32))
    assert np.array_equal(log_probs(scores.tolist(), lse.tolist()), lp)          # sequences are taken as float32
    with pytest.raises(RuntimeError):
        log_probs(scores, lse[:1])
    with pytest.raises(RuntimeError):
        probs(scores[0], lse)


def test_exports_and_arity(lib):
    from ader_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "ader_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, header)
        assert m, name
        assert len(_lib._SIGS[name]) == len(m.group(1).split(",")), name
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
    assert len(_lib._SIGS["ader_topk_items_stats"]) == len(_lib._SIGS["ader_topk_items"]) + 3      # + spart, lse, entropy
    assert len(_lib._SIGS["ader_row_stats"]) == 11 and len(_lib._SIGS["ader_row_stats_floats"]) == 2
    lib.ader_row_stats_floats.argtypes = lib.ader_topk_ranges.argtypes = [ctypes.c_int, ctypes.c_int]
    for N, Bp in ((1, 64), (650, 128), (40000, 128), (1_000_000, 1024), (33, 64)):
        ranges = lib.ader_topk_ranges(N, Bp)
        assert 8 <= ranges <= 256                          # k_stats_merge holds a row's ranges in LDS: at most 256
        assert lib.ader_row_stats_floats(N, Bp) == ranges * Bp * 4
    src = open(os.path.join(root, "ader_amd", "csrc", "topk_stats.hip")).read()
    assert "k_topk_tile_stats" in src and "k_row_stats" in src and "atomicAdd" not in src


def test_operators_trace_under_fake_tensors(lib):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb = torch.empty(5, 150), torch.empty(1001, 150)
        seen = torch.empty(5, 50, dtype=torch.int32)
        for s in (None, seen):
            items, scores, lse, ent = torch.ops.ader.topk_items_stats(rep, emb, s, 1000, 20)
            assert tuple(items.shape) == (5, 20) and items.dtype == torch.int32
            assert tuple(scores.shape) == (5, 20) and scores.dtype == torch.float32
            assert tuple(lse.shape) == tuple(ent.shape) == (5,) and lse.dtype == ent.dtype == torch.float32
        lse, ent = torch.ops.ader.row_stats(rep, emb, 1000)
        assert tuple(lse.shape) == tuple(ent.shape) == (5,) and lse.dtype == ent.dtype == torch.float32


# ------------------------------------------------------------------------------------------------ emulation of accumulate and merge
EMPTY = (F(-np.inf), F(0), F(0))


def move(st, mn):
    """stat_move, float32: a lane's running state restated at maximum mn >= m; an empty state (l == 0) is skipped, so -inf never
    meets 0."""
    m, l, u = st
    if l > 0:
        d = F(m - mn)
        e = np.exp(d, dtype=F)
        u = F(e * F(F(d * l) + u))
        l = F(l * e)
    return F(mn), l, u


def add4(st, v):
    """stat_add4: up to 4 logits enter a lane's state (the kernel's mask leaves out items past the row's last)."""
    if len(v) == 0:
        return st
    mt = F(v.max())
    if mt > st[0]:
        st = move(st, mt)
    m, l, u = st
    for s in v:
        t = F(s - m)
        e = np.exp(t, dtype=F)
        l = F(l + e)
        u = F(F(e * t) + u)
    return m, l, u


def move_d(st, mn):
    """stat_move_d: a float32 state moved to maximum mn >= m in double -> (L, U); an empty state gives (0, 0)."""
    m, l, u = st
    if not l > 0:
        return 0.0, 0.0
    d = float(m) - float(mn)
    e = math.exp(d)
    return e * float(l), e * (d * float(l) + float(u))


def join(states):
    """What joins states (the 16 lanes of a range, the ranges of a row): all moved to their common maximum and added in the given
    order, in double -> (m float32, L, U)."""
    mx = F(max(st[0] for st in states))
    L = U = 0.0
    for st in states:
        dl, du = move_d(st, mx)
        L, U = L + dl, U + du
    return mx, L, U


def readout(mx, L, U):
    ll = math.log(L)
    return F(float(mx) + ll), F(ll - U / L)


def emulate(s, bounds):
    """One row of float32 logits s over the item ranges [bounds[i], bounds[i+1]) (empty ones allowed): per range 64-item tiles, 16
    float32 lane states (4 waves mw x 4 lanes q), a lane owning items 16 mw + 4 q .. + 3 of every tile; the lanes joined in double,
    the partial rounded to float32; the ranges joined in double in ascending order -> (lse, entropy), float32."""
    parts = []
    for lo, hi in zip(bounds, bounds[1:]):
        lanes = [EMPTY] * 16
        for t0 in range(lo, hi, 64):
            for i in range(16):
                a = t0 + 4 * i
                lanes[i] = add4(lanes[i], s[a:min(a + 4, hi)] if a < hi else s[:0])
        mx, L, U = join(lanes)
        parts.append((mx, F(L), F(U)))
    return readout(*join(parts))



def reference(s):
    s = s.astype(np.float64)
    m = s.max()
    lse = m + np.log(np.exp(s - m).sum())
    p = np.exp(s - lse)
    return lse, -(p * (s - lse)).sum()


def floor_partition(N, ranges):
    """tile_walk's partition: the floor partition of the 64-item tiles into `ranges` ranges, in items, the last cut at N."""
    nt = (N + 63) // 64
    return [min(N, 64 * (r * nt // ranges)) for r in range(ranges)] + [N]


@pytest.mark.parametrize("sigma", [0.6, 3.0])
@pytest.mark.parametrize("N,ranges", [(1, 8), (33, 8), (650, 8), (650, 16), (4097, 8), (4097, 64), (20000, 8), (20000, 256)])
def test_any_partition_agrees_with_float64_within_the_cap(N, ranges, sigma):
    rs = np.random.RandomState(N + ranges)
    s = (rs.standard_normal(N) * sigma).astype(F)
    ref = reference(s)
    bounds = floor_partition(N, ranges)
    assert len(bounds) == ranges + 1 and (N >= 64 * ranges or any(a == b for a, b in zip(bounds, bounds[1:])))      # empty ranges occur
    cuts = sorted(rs.randint(0, N + 1, size=5).tolist())
    for b in (bounds, [0, N], [0, 0] + cuts + [N, N]):       # the kernel's partition, one range, ragged cuts with empty ends
        lse, ent = emulate(s, b)
        assert abs(float(lse) - ref[0]) <= CAP and abs(float(ent) - ref[1]) <= CAP, (b[:4], lse, ent, ref)


def test_the_empty_state_is_the_identity_of_the_merge():
    rs = np.random.RandomState(0)
    st = add4(EMPTY, (rs.standard_normal(4) * 3).astype(F))
    alone = join([st])
    assert alone == (st[0], float(st[1]), float(st[2]))      # moved by d = 0: e = 1, the sums keep their value
    for states in ([st, EMPTY], [EMPTY, st], [EMPTY] * 7 + [st] + [EMPTY] * 8):
        assert join(states) == alone
    e = join([EMPTY, EMPTY])
    assert np.isneginf(e[0]) and e[1] == 0.0 and e[2] == 0.0 and not np.isnan(e).any()      # padding rows, empty ranges: no NaN
    assert all(np.array_equal(F(x).view(np.int32), F(y).view(np.int32)) for x, y in zip(add4(EMPTY, st[:0]), EMPTY))
    a, b = add4(EMPTY, np.array([1.5, -2.0], dtype=F)), add4(EMPTY, np.array([7.25], dtype=F))
    assert join([a, b]) == join([b, a])                      # a pair commutes bit for bit: the lanes of a row end with one sum
    s = (rs.standard_normal(300) * 2).astype(F)
    with_empty = emulate(s, [0, 0, 100, 100, 300, 300])      # empty ranges between, before and after change no bit
    assert with_empty == emulate(s, [0, 100, 300])
    one = emulate(np.array([-3.75], dtype=F), [0, 1, 1])     # N = 1: lse has the score's bits, the entropy is exactly 0
    assert one[0] == F(-3.75) and one[1] == 0.0



def test_a_dominant_logit_gives_no_entropy_and_the_naive_form_does_not():
    """Why (m, l, u): entropy = log l - u / l adds terms of one sign and keeps a small entropy to its own precision; lse - sum p s
    subtracts two numbers of the size of the dominant logit, so what comes out is their rounding, a multiple of ulp(|s_max|)."""
    rs = np.random.RandomState(1)
    for N, top in ((650, 45.0), (4097, 173.0), (20000, 611.0)):
        s = (rs.standard_normal(N) * 0.6).astype(F)
        s[N // 3] = F(top + rs.rand())                       # at least 40 above every other logit
        lse, ent = emulate(s, floor_partition(N, 16))
        ref = reference(s)
        assert ref[1] < 1e-12 and 0.0 <= float(ent) < 1e-6
        assert abs(float(lse) - ref[0]) <= 2.0 ** -24 * abs(ref[0])
    # one item 17 below the dominant one, the rest out of reach: the entropy is e^-17 (1 + 17) = 7.5e-7.  The mass e^-17 = 4.1e-8 is
    # below half an ulp of 1, so lse is the dominant logit itself in float32; but e^-17 * 7983 = 3.3e-4 is above half an ulp of 8000
    # (2.4e-4), and the naive form's sum p s, met in the walk's order, lands one ulp above lse
    N = 650
    s = np.full(N, 8000.0 - 60.0, dtype=F)
    s[100], s[N - 1] = F(8000.0 - 17.0), F(8000.0)
    ref = reference(s)
    assert 7.0e-7 < ref[1] < 8.0e-7
    for ranges in (8, 16):
        lse, ent = emulate(s, floor_partition(N, ranges))
        assert lse == F(8000.0) and abs(float(ent) - ref[1]) < 1e-7 and float(ent) < 1e-6
    p = np.exp((s - lse).astype(F), dtype=F)
    acc = F(0)
    for x in (p * s).astype(F):
        acc = F(acc + x)
    naive = F(lse - acc)
    assert abs(float(naive)) > 1e-4                          # -2^-11: one ulp of 8000, 650 times the entropy
