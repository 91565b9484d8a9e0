"""Exact top-K recommendation for wide answers, k up to 1024 (Engine.recommend_wide, Ader.recommend, torch.ops.ader.topk_items_wide,
ader_topk_items_wide: slab and select, csrc/topk.hip).  The contract is Engine.recommend's: items ==
stable_argsort(-Engine.logits)[:, :k] + 1 with the gathered device logits as scores, bit for bit, order (score descending, item id
ascending), item 0 / -inf padding.  No tolerance anywhere.  Every contract case asserts overflowed_rows == 0 and max_list <= cap, so
the exact fallback of recommend_wide cannot stand in for the kernels (tests/test_topk_wide_host.py holds the premise: Gaussian operands
at these shapes leave every list within cap)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine(item_num, T, H, L, heads, seed=0, **kw):
    from ader_amd.engine import Engine
    kw.setdefault("logits_dtype", "f32")
    eng = Engine(item_num, maxlen=T, hidden_units=H, num_blocks=L, num_heads=heads, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed + 11)
    for k in eng.layout:
        base = k.split(".")[-1]
        shp = eng.layout[k][1]
        if base.endswith("_b") or base in ("bq", "bk", "bv", "b1", "b2"):
            eng.param(k).copy_(torch.randn(shp, generator=g) * 0.1)
        elif base.endswith("_g"):
            eng.param(k).copy_(1 + torch.randn(shp, generator=g) * 0.1)
        elif base in ("wq", "wk", "wv", "w1", "w2"):
            eng.param(k).copy_(torch.randn(shp, generator=g) * (1.0 / np.sqrt(shp[0])))
        elif base == "emb":
            eng.param(k).copy_(torch.randn(shp, generator=g) * 0.05)
    eng.refresh_shadow()
    return eng


def _seqs(rs, B, T, lo, hi):
    """Sessions of random length over the ids lo..hi."""
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(lo, hi + 1, size=ln)
    return seq


# item_num, T, H, L, heads, B, N, k, cap (None: the default, ader_topk_wide_cap())
SHAPES = [(700, 50, 150, 2, 1, 70, 650, 100, 256),            # many one-tile slabs, N no multiple of 64, two row chunks
          (1000, 50, 150, 2, 3, 130, 777, 65, 192),           # three chunks, three heads, the smallest wide k
          (5000, 20, 150, 1, 1, 65, 4097, 1024, 4096),        # kmax, the default cap, a final one-item slab
          (64, 8, 12, 1, 1, 3, 33, 100, 192),                 # k > N: padding, more of it with exclusion
          (2000, 20, 150, 1, 1, 1030, 1999, 70, None),        # over MAX_ROWS: two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000, 300, 1024),       # many slabs of growing size, thresholds carried from slab to slab
          (20000, 20, 150, 1, 1, 260, 20000, 64, None)]       # five chunks: the slabs after the first hold more tiles than a chunk
#                                                               has workgroups, so a workgroup walks several tiles under a threshold


def _reference(lg, seen, k, exclude):
    """The contract in numpy: lg [n,N] scores, seen [n,S] ids (0 = none, ids above N ignored) -> (items int32 [n,k], scores float32 [n,k])."""
    lg = np.array(lg, dtype=np.float32)
    n, N = lg.shape
    if exclude:
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


def _assert_same(got, ref, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == ref[0].shape == got[1].shape, what
    assert np.array_equal(got[0], ref[0]), what
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.int32), np.ascontiguousarray(ref[1]).view(np.int32)), what


def _capmax():
    from ader_amd._lib import call
    return call("ader_topk_wide_cap")


def _assert_unflagged(eng, n, N, k, cap):
    """The kernels alone produced the answer: no row was recomputed, and no list outgrew cap."""
    from ader_amd._lib import call
    cap = _capmax() if cap is None else cap
    st = eng.last_topk_stats
    assert set(st) == {"slabs", "rows", "max_list", "overflowed_rows", "fallback_rows"}
    assert st["overflowed_rows"] == 0 and st["fallback_rows"] == 0 and st["max_list"] <= cap, st
    assert st["rows"] == n and st["slabs"] == call("ader_topk_wide_slabs", N, k, cap, None, 0), st
    return st


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions and the device logits of SHAPES[i]: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N, k, cap = SHAPES[i]
    eng = _engine(item_num, T, H, L, heads)
    seq = _seqs(np.random.RandomState(6 + i), B, T, 1, N)
    lg = eng.logits(seq, N).cpu().numpy()
    lg.setflags(write=False)
    seq.setflags(write=False)
    return eng, seq, lg, N, k, cap


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_items_are_the_head_of_the_stable_argsort_of_the_device_logits(i, exclude):
    eng, seq, lg, N, k, cap = _case(i)
    got = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
    st = _assert_unflagged(eng, seq.shape[0], N, k, cap)
    _assert_same(got, _reference(lg, seq, k, exclude))
    if i == 0:
        assert st["slabs"] == 8 and st["max_list"] > k      # [0, 256), then one tile each: lists that grow past k and are cut
    if i == 2:
        assert st["slabs"] == 2                             # items [0, 4096) and the one-item slab
    if i == 3:
        assert st["slabs"] == 1 and st["max_list"] == 0 and (got[0][:, N:] == 0).all() and np.isneginf(got[1][:, N:]).all()
    if i == 5:
        assert st["slabs"] > 20
    if i == 6:
        assert st["slabs"] == 4 and (16384 - 8192) // 64 > 256 // ((seq.shape[0] + 63) // 64)      # 128 tiles over 51 workgroups a chunk


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("i", [0, 4])
def test_narrow_k_returns_the_bytes_of_recommend(i, k, exclude):
    eng, seq, lg, N, _, cap = _case(i)
    want = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="f32")
    got = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
    _assert_unflagged(eng, seq.shape[0], N, k, cap)
    _assert_same(got, want)
    if i == 0:
        _assert_same(eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=k + 64 + (-k) % 64), want, "the smallest cap")
        _assert_unflagged(eng, seq.shape[0], N, k, k + 64 + (-k) % 64)


def test_rank_of_the_jth_item_is_j():
    eng, seq, lg, N, _, cap = _case(0)
    k = 100
    items, _ = eng.recommend_wide(seq, k, N, cap=cap)
    _assert_unflagged(eng, seq.shape[0], N, k, cap)
    assert (items > 0).all()
    ranks = eng.rank_targets(np.repeat(seq, k, axis=0), items.reshape(-1), N, dtype="f32")
    assert np.array_equal(ranks.reshape(-1, k), np.tile(np.arange(k, dtype=np.int32), (seq.shape[0], 1)))


@pytest.mark.parametrize("exclude", [False, True])
def test_planted_ties_across_slab_boundaries_and_the_kth_place(exclude):
    """Table rows copied onto items on both sides of the slab boundaries (ids 256 | 257, 320 | 321, ... are the last item of one slab and
    the first of the next at N = 650, k = 100, cap = 256) and onto the items of places k - 1 .. k + 2 of row 0, plus a block of zero
    rows (score +0 for every session): the tie rule decides what is kept, slab by slab."""
    from ader_amd._lib import call
    item_num, T, H, L, heads, B, N, k, cap = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1].copy()
    seq[0, -7:] = [660, 651, 700, 688, 660, 671, 699]               # row 0 over ids above N: its representation survives the planting
    seq[0, :-7] = 0
    emb = eng.param("emb")
    emb[401:421] = 0.0                                              # the zero rows first: row 0's places below are counted with them
    eng.refresh_shadow()
    order0 = np.argsort(-eng.logits(seq[:1], N).cpu().numpy()[0], kind="stable") + 1
    bounds = np.zeros(64, dtype=np.int32)
    ns = call("ader_topk_wide_slabs", N, k, cap, bounds.ctypes.data, 64)
    bounds = bounds[:ns + 1].tolist()
    assert bounds[:4] == [0, 256, 320, 384]
    top = int(order0[0])
    edge = [i for b in bounds[1:4] for i in (b, b + 1) if i != top]   # 1-based ids b | b + 1: either side of the boundary after item b
    rest = [int(x) for x in order0 if int(x) != top and int(x) not in edge]
    lead = sorted(edge + [top])
    kth = rest[k - 2 - len(lead):k + 2 - len(lead)]                  # with the boundary ties in front: places k - 1 .. k + 2 of row 0
    assert not set(range(401, 421)) & set(lead + kth)
    for j in edge:
        emb[j] = emb[top]
    for j in kth[1:]:
        emb[j] = emb[kth[0]]
    eng.refresh_shadow()
    lg = eng.logits(seq, N).cpu().numpy()
    assert len(set(lg[0, np.array(edge + [top]) - 1].view(np.int32).tolist())) == 1
    assert (lg[:, 400:420].view(np.int32) == 0).all()
    ref = _reference(lg, seq, k, exclude)
    sc0 = _reference(lg, seq, N, exclude)[1][0]
    assert sc0[k - 2] == sc0[k - 1] == sc0[k] == sc0[k + 1], "row 0's tie straddles the k-th place"
    got = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
    _assert_unflagged(eng, seq.shape[0], N, k, cap)
    _assert_same(got, ref)
    assert list(got[0][0, :len(lead)]) == lead and list(got[0][0, k - 2:]) == sorted(kth)[:2]


def test_total_tie_returns_the_first_ids():
    item_num, T, H, L, heads, B, N, k, cap = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    emb = eng.param("emb")
    emb[1:N + 1] = emb[1].clone()
    eng.refresh_shadow()
    for exclude in (False, True):
        items, scores = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
        st = _assert_unflagged(eng, seq.shape[0], N, k, cap)
        assert st["max_list"] == k or exclude                       # nothing after slab 0 beats a threshold it ties with
        for b in range(B):
            unseen = [n for n in range(1, N + 1) if not (exclude and n in set(seq[b].tolist()))][:k]
            assert list(items[b]) == unseen
        _assert_same((items, scores), _reference(eng.logits(seq, N).cpu().numpy(), seq, k, exclude))


# ---------------------------------------------------------------------------------------------- overflow
def _ascending(B, N, H, rs):
    """Scores ascending in the item id for every row: table row n = (n / N) u, rep rows = u."""
    u = rs.standard_normal(H).astype(np.float32)
    emb = np.zeros((N + 1, H), dtype=np.float32)
    emb[1:] = (np.arange(1, N + 1, dtype=np.float32) / np.float32(N))[:, None] * u[None, :]
    rep = np.tile(u, (B, 1))
    return rep, emb


def test_overflow_flags_every_row_and_writes_nothing_outside_the_list():
    """Every item beats every threshold, so a slab larger than cap - k overflows every row's list (tests/test_topk_wide_host.py:
    the schedule of N = 8300, k = 100, cap = 256 has such a slab).  The list buffer has a guard row of cap keys on either side, filled
    with a sentinel: the guards keep their bytes, as do the slots of the padding rows."""
    import ader_amd.ops  # noqa: F401
    from ader_amd import _lib
    B, N, H, k, cap = 70, 8300, 12, 100, 256
    rep, emb = _ascending(B, N, H, np.random.RandomState(8))
    dev = torch.device("cuda")
    rep_d, emb_d = torch.from_numpy(rep).to(dev), torch.from_numpy(emb).to(dev)
    items, scores, over = torch.ops.ader.topk_items_wide(rep_d, emb_d, None, N, k, cap)
    assert tuple(over.shape) == (B,) and bool((over != 0).all())
    Bp = 128
    sentinel = 0x5A5A5A5A5A5A5A5A
    lst = torch.full(((Bp + 2) * cap,), sentinel, dtype=torch.int64, device=dev)
    ncol = torch.zeros(Bp, dtype=torch.int32, device=dev)
    ncol[:B] = N
    cnt, stat = (torch.full((Bp,), 7, dtype=torch.int32, device=dev) for _ in range(2))
    thr = torch.full((Bp,), 7, dtype=torch.int64, device=dev)
    diag = torch.full((2,), 7, dtype=torch.int32, device=dev)
    it, sc = torch.zeros(B, k, dtype=torch.int32, device=dev), torch.zeros(B, k, device=dev)
    _lib.call("ader_topk_items_wide", _lib.ptr(rep_d), _lib.ptr(emb_d), B, Bp, H, N, _lib.ptr(ncol), None, 0, k, cap,
              _lib.ptr(lst[cap:]), _lib.ptr(cnt), _lib.ptr(thr), _lib.ptr(stat), _lib.ptr(diag), _lib.ptr(it), _lib.ptr(sc),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lst = lst.cpu().numpy().reshape(Bp + 2, cap)
    assert (lst[0] == sentinel).all() and (lst[-1] == sentinel).all(), "a guard row was written"
    assert (lst[1 + B:] == sentinel).all(), "a padding row's list was written"
    assert (lst[1:1 + B] != sentinel).any()
    stat, diag = stat.cpu().numpy(), diag.cpu().numpy()
    assert (stat[:B] != 0).all() and (stat[B:] == 0).all()
    assert diag[1] == B and diag[0] > cap


def test_engine_recomputes_overflowed_rows_exactly():
    """Row 0's session holds ids above N only, so planting the rows 1..N leaves its representation as it is: table row n = (n / N) rep_0.
    Row 0's scores ascend in the id (rep_0 . rep_0 > 0) and its list overflows; every row's answer is still the reference."""
    item_num, N, T, H, k, cap = 8400, 8300, 20, 64, 100, 256
    eng = _engine(item_num, T, H, 1, 1)
    seq = _seqs(np.random.RandomState(21), 70, T, 1, item_num)            # rows 1..: any id, so overflowed rows have seen ids to drop
    seq[0] = _seqs(np.random.RandomState(22), 1, T, N + 1, item_num)[0]
    rep0 = eng.encode(seq)[0].clone()
    emb = eng.param("emb")
    emb[1:N + 1] = (torch.arange(1, N + 1, dtype=torch.float32, device=emb.device) / N)[:, None] * rep0[None, :]
    eng.refresh_shadow()
    assert torch.equal(eng.encode(seq)[0], rep0)
    lg = eng.logits(seq, N).cpu().numpy()
    assert (np.diff(lg[0]) > 0).all()
    for exclude in (False, True):
        got = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
        st = eng.last_topk_stats
        assert st["overflowed_rows"] > 0 and st["fallback_rows"] == st["overflowed_rows"] and st["max_list"] > cap, st
        _assert_same(got, _reference(lg, seq, k, exclude))
    assert list(got[0][0]) == list(range(N, N - k, -1))
    eng.check_status()


# ---------------------------------------------------------------------------------------------- arguments, model, repeatability
def test_errors():
    """k in (0, 1025), cap in (k + 63, 4160, 200), N in (0, item_num + 1): RuntimeError from the Engine and the operator, -2 from the
    launcher (which is not told item_num: there N = 0 only)."""
    import ader_amd.ops  # noqa: F401
    from ader_amd import _lib
    eng, seq, lg, N, k, cap = _case(3)
    kmax = _lib.call("ader_topk_wide_kmax")
    assert kmax == 1024 and _capmax() == 4096
    bad = [dict(k=0), dict(k=kmax + 1), dict(cap=k + 63), dict(cap=4160), dict(cap=200), dict(N=0), dict(N=eng.item_num + 1)]
    dev = eng.device
    rep = torch.zeros(64, eng.H, device=dev)
    emb = eng.param("emb")
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    lst = torch.zeros(64 * 4224, dtype=torch.int64, device=dev)
    cnt, stat, thr = (torch.zeros(64, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int64))
    diag = torch.zeros(2, dtype=torch.int32, device=dev)
    items, scores = torch.zeros(64, kmax + 1, dtype=torch.int32, device=dev), torch.zeros(64, kmax + 1, device=dev)
    for b in bad:
        a = dict(k=k, cap=cap, N=N)
        a.update(b)
        with pytest.raises(RuntimeError):
            eng.recommend_wide(seq, a["k"], a["N"], cap=a["cap"])
        with pytest.raises(RuntimeError):
            torch.ops.ader.topk_items_wide(rep, emb, None, a["N"], a["k"], a["cap"])
        if a["N"] <= eng.item_num:
            with pytest.raises(_lib.AderHipError, match="code -2"):
                _lib.call("ader_topk_items_wide", _lib.ptr(rep), eng._pp["emb"], 64, 64, eng.H, a["N"], _lib.ptr(ncol), None, 0, a["k"],
                          a["cap"], _lib.ptr(lst), _lib.ptr(cnt), _lib.ptr(thr), _lib.ptr(stat), _lib.ptr(diag), _lib.ptr(items),
                          _lib.ptr(scores), torch.cuda.current_stream().cuda_stream)
    for bad_k in (0, 65):                                   # the narrow calls keep their limit
        with pytest.raises(RuntimeError):
            eng.recommend(seq, bad_k, N)
    eng.check_status()


def test_ader_recommend_takes_the_wide_path_above_64_and_raises_with_candidates():
    import types

    from ader_amd.model import Ader
    item_num, N, T = 400, 350, 50
    args = types.SimpleNamespace(maxlen=T, hidden_units=150, num_blocks=2, num_heads=1, random_seed=0, dropout_rate=0.3, l2_emb=0.0,
                                 disable_distillation=False, logits_dtype="f32")
    model = Ader(item_num, args)
    eng = model.engine
    seq = _seqs(np.random.RandomState(2), 9, T, 1, N)
    lg = eng.logits(seq, N).cpu().numpy()
    for exclude in (False, True):
        for dtype in (None, "f32", "x3"):
            got = model.recommend(seq, 65, N, exclude_seen=exclude, dtype=dtype)
            assert set(eng.last_topk_stats) >= {"slabs", "max_list"} and eng.last_topk_stats["overflowed_rows"] == 0
            _assert_same(got, _reference(lg, seq, 65, exclude))
    _assert_same(model.recommend(seq, 64, N), _reference(lg, seq, 64, False))
    with pytest.raises(RuntimeError):
        model.recommend(seq, 65, N, dtype="f16")
    with pytest.raises(RuntimeError):
        model.recommend(seq, 65, N, candidates=np.arange(1, 200))
    with pytest.raises(RuntimeError):
        model.recommend(seq, 1025, N)


@pytest.mark.parametrize("exclude", [False, True])
def test_calls_repeat_and_rows_are_independent(exclude):
    eng, seq, lg, N, k, cap = _case(1)
    a = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
    b = eng.recommend_wide(seq, k, N, exclude_seen=exclude, cap=cap)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    perm = np.random.RandomState(3).permutation(seq.shape[0])
    c = eng.recommend_wide(np.ascontiguousarray(seq[perm]), k, N, exclude_seen=exclude, cap=cap)
    assert np.array_equal(c[0], a[0][perm])
    assert np.array_equal(np.ascontiguousarray(c[1]).view(np.int32), np.ascontiguousarray(a[1][perm]).view(np.int32))
