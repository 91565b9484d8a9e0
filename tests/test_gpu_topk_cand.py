"""Top-K recommendation over a candidate item list (Engine.recommend_among, Ader.recommend(candidates=...), torch.ops.ader.topk_items_cand,
ader_topk_items_cand).  The contract is ader_topk_items' over a smaller set: items == stable_argsort(-L)[:, :k] + 1 and the gathered
scores bit for bit, where L is Engine.logits with every non-candidate column (and, under exclude_seen, every seen column) at -inf.
No tolerance anywhere: items and score bit patterns are compared with array_equal."""
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


def _seqs(rs, B, T, n_items):
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


# item_num, T, H, L, heads, B, N, k
SHAPES = [(700, 50, 150, 2, 1, 70, 650, 20),          # rows over one chunk, N no multiple of 64
          (300, 20, 64, 1, 2, 9, 300, 10),            # small batch, two heads
          (1000, 50, 150, 2, 3, 130, 777, 64),        # three chunks, k at K_MAX
          (64, 8, 12, 1, 1, 3, 33, 64),               # k > N: padding
          (2000, 20, 150, 1, 1, 1030, 1999, 5),       # over MAX_ROWS: two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000, 20)]      # a workgroup walks several tiles


def _reference(lg, cand, seen, k, exclude):
    """The contract in numpy: lg [n,N] scores, cand = ids in [1, N], seen [n,S] ids (0 = none, ids above N ignored) -> (items, scores)."""
    lg = np.array(lg, dtype=np.float32)
    n, N = lg.shape
    out = np.ones(N, dtype=bool)
    out[np.asarray(cand, dtype=np.int64) - 1] = False
    lg[:, out] = -np.inf
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
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.int32), ref[1].view(np.int32)), what


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions and the device logits of SHAPES[i]: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N, k = SHAPES[i]
    eng = _engine(item_num, T, H, L, heads)
    seq = _seqs(np.random.RandomState(6 + i), B, T, N)
    lg = eng.logits(seq, N).cpu().numpy()
    lg.setflags(write=False)
    seq.setflags(write=False)
    return eng, seq, lg, N, k


def _patterns(i):
    """(name, list as handed to recommend_among, its ids within [1, N]) for SHAPES[i]."""
    item_num, N = SHAPES[i][0], SHAPES[i][6]
    rs = np.random.RandomState(40 + i)
    out = [("third", np.sort(rs.choice(N, size=max(N // 3, 1), replace=False)) + 1)]
    perm = rs.permutation(N) + 1
    for M in (0, 1, 63, 64, 65, 129):                  # an empty list, a single entry, both sides of a tile edge; M < k: padding
        out.append(("first %d of a permutation" % M, np.sort(perm[:M])))
    out.append(("1..64 and every 97th", np.unique(np.concatenate([np.arange(1, min(64, N) + 1), np.arange(97, N + 1, 97)]))))
    above = np.arange(N + 1, item_num + 1)[::7]        # ids in (N, item_num]: legal, ignored (none where N == item_num)
    out.append(("ids above N", np.concatenate([out[0][1][::2], above])))
    if i == 5:
        out.append(("5000 spread", np.arange(4, N + 1, 8)))
        out.append(("20000 spread", np.arange(1, N + 1, 2)))
    return [(name, c.astype(np.int64), c[c <= N]) for name, c in out]


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_all_ids_equal_the_contiguous_walk_and_the_masked_argsort(i, exclude):
    eng, seq, lg, N, k = _case(i)
    full = np.arange(1, N + 1)
    got = eng.recommend_among(seq, k, full, N, exclude_seen=exclude)
    _assert_same(got, eng.recommend(seq, k, N, exclude_seen=exclude), "against k_topk_tile")
    _assert_same(got, _reference(lg, full, seq, k, exclude))
    assert eng.last_topk_stats is None


@functools.lru_cache(maxsize=None)
def _three_entry_case():
    """B = 70: two chunks, six rows in the second.  N = 8,300: 130 tiles over ader_topk_ranges = 128 ranges per chunk, so two workgroups
    per chunk carry a row's threshold from one tile into the next; k = 64 = K_MAX."""
    B, N, T = 70, 8300, 20
    eng = _engine(N, T, 150, 1, 1)
    seq = _seqs(np.random.RandomState(77), B, T, N)
    lg = eng.logits(seq, N).cpu().numpy()
    lg.setflags(write=False)
    seq.setflags(write=False)
    return eng, seq, lg, N, 64


@pytest.mark.parametrize("exclude", [False, True])
def test_the_three_entry_points_of_the_shared_row_buffer_return_equal_bytes(exclude):
    """recommend (k_topk_tile), recommend_among over all ids (k_topk_cand) and recommend_wide (k_topk_wide_tile) share the walk, the
    tile stream and -- the first two -- the row buffer of csrc/logit_tile.h: the same bytes, and the stable argsort of the logits."""
    from ader_amd._lib import call
    eng, seq, lg, N, k = _three_entry_case()
    assert (N + 63) // 64 == 130 and call("ader_topk_ranges", N, 128) == 128
    full = np.arange(1, N + 1)
    tile = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="f32")
    among = eng.recommend_among(seq, k, full, N, exclude_seen=exclude)
    wide = eng.recommend_wide(seq, k, N, exclude_seen=exclude)
    assert eng.last_topk_stats["overflowed_rows"] == 0             # the wide rows are k_topk_wide_tile's, not a recomputation
    for name, got in (("recommend_among", among), ("recommend_wide", wide)):
        assert got[0].tobytes() == tile[0].tobytes() and got[1].tobytes() == tile[1].tobytes(), name
    _assert_same(tile, _reference(lg, full, seq, k, exclude))


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_candidate_patterns_are_the_head_of_the_masked_stable_argsort(i, exclude):
    from ader_amd._lib import call
    eng, seq, lg, N, k = _case(i)
    Bp = (min(seq.shape[0], eng.MAX_ROWS) + 63) // 64 * 64
    for name, given, inside in _patterns(i):
        got = eng.recommend_among(seq, k, given, N, exclude_seen=exclude)
        _assert_same(got, _reference(lg, inside, seq, k, exclude), name)
        if len(inside) < k:
            assert (got[0][:, len(inside):] == 0).all() and np.isneginf(got[1][:, len(inside):]).all(), name
        assert np.isin(got[0][got[0] > 0], inside).all(), name
        if name == "5000 spread":
            assert len(inside) == 5000
        if name == "20000 spread":
            # a workgroup walks several gathered tiles: thresholds carry over, compaction after the first.  (5,000 ids are 79 tiles
            # against ader_topk_ranges(5000, 128) = 80 ranges -- at most one tile per workgroup -- so the assertion sits on a list
            # long enough for it to hold.)
            assert (len(inside) + 63) // 64 > call("ader_topk_ranges", len(inside), Bp)


def test_planted_ties_lead_in_ascending_id_and_a_tied_non_candidate_stays_out():
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    t = int(np.argmax(_case(0)[2][0])) + 1             # row 0's best item (the same seed: the same parameters as the shared engine)
    emb = eng.param("emb")
    tied = sorted([t] + [j for j in (3, 200, 411, N - 2, 500) if j != t][:4])      # spread over the catalog's tiles
    for j in tied:
        emb[j] = emb[t]
    eng.refresh_shadow()
    left_out = tied[2]
    rs = np.random.RandomState(9)
    cand = np.unique(np.concatenate([rs.choice(N, size=150, replace=False) + 1, tied]))
    cand = cand[cand != left_out]
    lg = eng.logits(seq, N).cpu().numpy()
    assert len(set(lg[0, np.array(tied) - 1].view(np.int32).tolist())) == 1
    got = eng.recommend_among(seq, k, cand, N)
    _assert_same(got, _reference(lg, cand, seq, k, False))
    four = [j for j in tied if j != left_out]
    assert list(got[0][0, :4]) == four and len(set(got[1][0, :4].tolist())) == 1
    assert left_out not in got[0][0].tolist()


def _op(rep, emb, cand, seen, N, k):
    import ader_amd.ops  # noqa: F401
    dev = torch.device("cuda")
    as_dev = lambda x, dt: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=dt)).to(dev)
    s = None if seen is None else as_dev(seen, np.int32)
    items, scores = torch.ops.ader.topk_items_cand(as_dev(rep, np.float32), as_dev(emb, np.float32), as_dev(cand, np.int32), s, N, k)
    return items.cpu().numpy(), scores.cpu().numpy()


def test_total_tie_returns_the_first_k_candidate_ids():
    rs = np.random.RandomState(2)
    B, N, H, k = 70, 650, 150, 20
    emb = (rs.standard_normal((N + 1, H)) * 0.05).astype(np.float32)
    rep = rs.standard_normal((B, H)).astype(np.float32)
    rep[::2] = 0.0                                     # all-zero rep rows: every score is +0
    cand = np.sort(rs.choice(N, size=300, replace=False)) + 1
    items, scores = _op(rep, emb, cand, None, N, k)
    for b in range(0, B, 2):
        assert list(items[b]) == cand[:k].tolist()
    assert (np.ascontiguousarray(scores[::2]).view(np.int32) == 0).all()
    lg = np.zeros((B, N), dtype=np.float32)
    _assert_same((items[::2], scores[::2]), _reference(lg[::2], cand, None, k, False))


def test_an_unsorted_list_with_duplicates_is_the_normalised_list():
    from ader_amd.engine.infer import candidate_ids
    eng, seq, lg, N, k = _case(0)
    rs = np.random.RandomState(12)
    raw = rs.randint(1, eng.item_num + 1, size=400)
    raw = np.concatenate([raw, raw[:50]])
    assert len(np.unique(raw)) < len(raw) and (np.diff(raw) < 0).any() and (raw > N).any()
    norm = candidate_ids(raw, N, eng.item_num)
    a = eng.recommend_among(seq, k, raw, N)
    for other in (norm, torch.from_numpy(raw), raw.tolist(), torch.from_numpy(raw.astype(np.int32)).to(eng.device)):
        b = eng.recommend_among(seq, k, other, N)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _assert_same(a, _reference(lg, norm, seq, k, False))


def test_raw_op_raises_on_a_list_that_is_not_strictly_ascending():
    eng, seq, lg, N, k = _case(0)
    rep, emb = eng.encode(seq), eng.param("emb")
    good = np.arange(5, 400, 3)                        # every id inside [1, N]: even a faulty kernel reads only inside the table
    for bad in (good[::-1].copy(), np.concatenate([good[:70], good[69:]]), np.concatenate([good[:100], good[:30]])):
        assert bad.min() >= 1 and bad.max() <= N
        with pytest.raises(RuntimeError, match="ascending"):
            _op(rep, emb, bad, None, N, k)
    _assert_same(_op(rep, emb, good, None, N, k), _reference(lg, good, seq, k, False))


@pytest.mark.parametrize("with_seen", [False, True])
def test_raw_op_ignores_ids_above_n(with_seen):
    eng, seq, lg, N, k = _case(0)                      # N = 650 of item_num = 700
    rep, emb = eng.encode(seq), eng.param("emb")
    cand = np.arange(2, eng.item_num + 1, 3)
    assert (cand > N).any() and cand.max() <= eng.item_num
    items, scores = _op(rep, emb, cand, seq if with_seen else None, N, k)
    assert items.max() <= N and (items > 0).all()
    _assert_same((items, scores), _reference(lg, cand[cand <= N], seq, k, with_seen))


def test_engine_raises_on_ids_outside_the_catalog_before_any_launch():
    eng, seq, lg, N, k = _case(3)
    for bad in ([0, 3], [-1, 3], [3, eng.item_num + 1], np.array([1.0, 2.0]), np.array([[1, 2]])):
        with pytest.raises(RuntimeError):
            eng.recommend_among(seq, 5, bad, N)
    eng.check_status()


@pytest.mark.parametrize("exclude", [False, True])
def test_calls_repeat_and_rows_are_independent(exclude):
    eng, seq, lg, N, k = _case(2)
    cand = _patterns(2)[0][1]
    a = eng.recommend_among(seq, k, cand, N, exclude_seen=exclude)
    b = eng.recommend_among(seq, k, cand, N, exclude_seen=exclude)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    perm = np.random.RandomState(3).permutation(seq.shape[0])
    c = eng.recommend_among(np.ascontiguousarray(seq[perm]), k, cand, N, exclude_seen=exclude)
    assert np.array_equal(c[0], a[0][perm])
    assert np.array_equal(np.ascontiguousarray(c[1]).view(np.int32), np.ascontiguousarray(a[1][perm]).view(np.int32))


def test_errors():
    from ader_amd import _lib
    eng, seq, lg, N, k = _case(3)
    kmax = _lib.call("ader_topk_kmax")
    cand = np.arange(1, N + 1, 2)
    for bad_k in (0, kmax + 1):
        with pytest.raises(RuntimeError):
            eng.recommend_among(seq, bad_k, cand, N)
    dev = eng.device
    M = len(cand)
    cand_d = torch.from_numpy(cand.astype(np.int32)).to(dev)
    rep = torch.zeros(64, eng.H, device=dev)
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    part = torch.zeros(_lib.call("ader_topk_ranges", M, 64) * 64 * (kmax + 1), dtype=torch.int64, device=dev)
    items = torch.zeros(64, kmax + 1, dtype=torch.int32, device=dev)
    scores = torch.zeros(64, kmax + 1, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.AderHipError, match="code -2"):
        _lib.call("ader_topk_items_cand", _lib.ptr(rep), eng._pp["emb"], 64, 64, eng.H, N, _lib.ptr(ncol), _lib.ptr(cand_d), M, None, 0,
                  kmax + 1, _lib.ptr(part), _lib.ptr(items), _lib.ptr(scores), _lib.ptr(status), torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == 0


@pytest.mark.parametrize("exclude", [False, True])
def test_x3_with_a_candidate_list_takes_the_f32_kernels(exclude):
    from ader_amd.engine.infer import rank_x3_supports
    eng, seq, lg, N, k = _case(0)
    assert rank_x3_supports(eng.H)                     # without a list this engine's "x3" call is the x3 path
    cand = _patterns(0)[0][1]
    eng.recommend(seq, k, N, dtype="x3")
    assert eng.last_topk_stats is not None
    a = eng.recommend_among(seq, k, cand, N, exclude_seen=exclude, dtype="x3")
    assert eng.last_topk_stats is None
    b = eng.recommend_among(seq, k, cand, N, exclude_seen=exclude, dtype="f32")
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    _assert_same(a, _reference(lg, cand[cand <= N], seq, k, exclude))
