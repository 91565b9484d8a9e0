"""Item lists that differ from row to row (Engine.score_items / recommend_per_row / rank_targets_per_row, their Ader forwarders,
torch.ops.ader.score_items / topk_items_rows / rank_of_target_rows, ader_score_items / ader_topk_items_rows / ader_rank_targets_rows,
Evaluator(negatives=...), --eval_negatives).  The reference is the device's own Engine.logits plus numpy: a listed item's score is the
logit's float32, a row's answer the head of the stable argsort of its logits with every unlisted (and, under exclude_seen, every seen)
column at -inf, a target's rank the count of tests/test_rowlist_host.py's oracle.  No tolerance anywhere: ids, ranks and score bit
patterns are compared with array_equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rowlist_host import oracle_ranks_rows  # noqa: E402

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


# item_num, T, H, L, heads, B, N
SHAPES = [(700, 50, 150, 2, 1, 70, 650),              # H no multiple of 4, rows over one 64-chunk
          (300, 20, 64, 1, 2, 9, 300),
          (64, 8, 12, 1, 1, 3, 33),                   # tiny H, C > N
          (2000, 20, 150, 1, 1, 1030, 1999),          # two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000)]          # gathers far apart
WIDTHS = (0, 1, 15, 16, 17, 63, 64, 65, 129, 300)     # both sides of a wave's 16 positions and of a 64-position tile
KS = (1, 20, 64)
IDS = range(len(SHAPES))


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions, targets and the device logits of SHAPES[i]: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N = SHAPES[i]
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(6 + i)
    seq = _seqs(rs, B, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)           # random ids in [1, N]: some inside a row's list, most outside
    pos[1::5] = seq[1::5, -1]                                      # ... and some among the row's own seen ids
    lg = eng.logits(seq, N).cpu().numpy()
    for a in (lg, seq, pos):
        a.setflags(write=False)
    return eng, seq, pos, lg, N


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _lists(i, C, seed):
    """Ragged lists for SHAPES[i] as a zero-padded [B, C] matrix, unsorted and with duplicates: row b has C entries (b % 3 != 0) or a random
    number of them, some of its own seq ids and of the targets among them, ids in (N, item_num] as well."""
    eng, seq, pos, lg, N = _case(i)
    rs = np.random.RandomState(seed + 31 * i + C)
    B = seq.shape[0]
    out = np.zeros((B, C), dtype=np.int64)
    for b in range(B):
        ln = C if b % 3 else int(rs.randint(0, C + 1))
        row = rs.randint(1, eng.item_num + 1, size=ln)
        own = seq[b][seq[b] > 0]
        m = min(len(own), ln // 2)
        row[:m] = own[:m]                                          # every row that has room holds some of its own seq ids
        if ln > m and b % 2:
            row[m] = pos[b]                                        # the target listed in every other row
        if ln > 3:
            row[-1] = row[0]                                       # a duplicate
        out[b, :ln] = rs.permutation(row)
    return out


def _sets(lists, N):
    return [np.unique(r[(r >= 1) & (r <= N)]) for r in lists]


def _reference_rows(lg, sets, seen, k, exclude):
    """_reference of tests/test_gpu_topk_cand.py with a mask per row: the head of the stable argsort of -lg with every column outside the
    row's set (and, under exclude, every seen column) at -inf."""
    lg = np.array(lg, dtype=np.float32)
    n, N = lg.shape
    keep = np.zeros((n, N), dtype=bool)
    for b in range(n):
        keep[b, sets[b] - 1] = True
        if exclude:
            s = seen[b][(seen[b] > 0) & (seen[b] <= N)]
            keep[b, s - 1] = False
    lg[~keep] = -np.inf
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
    assert np.array_equal(_bits(got[1]), _bits(ref[1])), what


# ------------------------------------------------------------------------------------------------ 1. score_items
@pytest.mark.parametrize("i", IDS)
def test_score_items_returns_the_bits_of_the_logits(i):
    eng, seq, pos, lg, N = _case(i)
    B = seq.shape[0]
    rs = np.random.RandomState(100 + i)
    for C in WIDTHS:
        items = rs.randint(-3, eng.item_num + 1, size=(B, C)).astype(np.int64)      # unsorted, duplicates, zeros, negatives, ids above N
        if C:
            items[:, 0] = N                                                          # item N itself
        if C > 1:
            items[::2, C // 2] = 0
        if C > 2:
            items[:, -1] = items[:, 1]
        got = eng.score_items(seq, items, N)
        assert got.dtype == np.float32 and got.shape == (B, C)
        live = (items >= 1) & (items <= N)
        ref = np.full((B, C), -np.inf, dtype=np.float32)
        rows = np.nonzero(live)[0]
        ref[live] = lg[rows, items[live] - 1]
        assert np.array_equal(_bits(got), _bits(ref)), C
        if C > 2:
            assert live[:, 0].all() and not live.all()
        for form in (torch.from_numpy(items), items.astype(np.int32)):
            assert np.array_equal(_bits(eng.score_items(seq, form, N)), _bits(ref)), C
        # the same rows scored alone, on the session forward the batch took ("auto" packing goes by a host batch's density, and the
        # packed session kernels round differently: a device slice under keep_density keeps the batch's choice)
        seq_d = eng._dev_i32(seq)
        kd, eng._step.keep_density = eng._step.keep_density, True
        try:
            for b in (0, B - 1):
                alone = eng.score_items(seq_d[b:b + 1], items[b:b + 1], N)
                assert np.array_equal(_bits(alone), _bits(ref[b:b + 1])), (C, b)
        finally:
            eng._step.keep_density = kd
    eng.check_status()


def test_score_items_errors():
    eng, seq, pos, lg, N = _case(2)
    for bad in (np.ones((seq.shape[0], 4)), np.ones(4, dtype=np.int32), np.ones((seq.shape[0] + 1, 4), dtype=np.int32)):
        with pytest.raises(RuntimeError):
            eng.score_items(seq, bad, N)
    for bad_n in (0, eng.item_num + 1):
        with pytest.raises(RuntimeError, match="max_item"):
            eng.score_items(seq, np.ones((seq.shape[0], 4), dtype=np.int32), bad_n)


# ------------------------------------------------------------------------------------------------ 2. recommend_per_row
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_recommend_per_row_is_the_head_of_the_masked_stable_argsort(i, exclude):
    eng, seq, pos, lg, N = _case(i)
    for C in WIDTHS:
        lists = _lists(i, C, 0)
        sets = _sets(lists, N)
        ref = _reference_rows(lg, sets, seq, max(KS), exclude)
        for k in KS:
            got = eng.recommend_per_row(seq, k, lists, N, exclude_seen=exclude)
            _assert_same(got, (np.ascontiguousarray(ref[0][:, :k]), np.ascontiguousarray(ref[1][:, :k])), (C, k))
        short = [b for b in range(len(sets)) if len(sets[b]) < max(KS)]
        assert short or C >= max(KS)
        for b in short[:5]:                                        # rows shorter than k: padding
            assert (got[0][b, len(sets[b]):] == 0).all() and np.isneginf(got[1][b, len(sets[b]):]).all()
        assert eng.last_topk_stats is None
    # ragged rows given as sequences are the padded matrix
    lists = _lists(i, 65, 0)
    rag = [r[r > 0].tolist() for r in lists]
    a, b = eng.recommend_per_row(seq, 20, rag, N, exclude_seen=exclude), eng.recommend_per_row(seq, 20, lists, N, exclude_seen=exclude)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    eng.check_status()


# ------------------------------------------------------------------------------------------------ 3. the existing entry points
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_all_ids_and_a_shared_list_equal_recommend_and_recommend_among(i, exclude):
    eng, seq, pos, lg, N = _case(i)
    B = seq.shape[0]
    k = 20
    full = np.broadcast_to(np.arange(1, N + 1, dtype=np.int32), (B, N))
    got = eng.recommend_per_row(seq, k, full, N, exclude_seen=exclude)
    ref = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="f32")
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    shared = np.unique(np.random.RandomState(50 + i).randint(1, eng.item_num + 1, size=max(N // 3, 1)))
    got = eng.recommend_per_row(seq, k, np.broadcast_to(shared, (B, len(shared))), N, exclude_seen=exclude)
    ref = eng.recommend_among(seq, k, shared, N, exclude_seen=exclude)
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()
    eng.check_status()


@pytest.mark.parametrize("i", IDS)
def test_the_retrieval_list_of_recommend_wide_through_the_re_ranking_calls(i):
    eng, seq, pos, lg, N = _case(i)
    w_items, w_scores = eng.recommend_wide(seq, 256, N)
    assert np.array_equal(_bits(eng.score_items(seq, w_items, N)), _bits(w_scores))       # padding (item 0) scores -inf, as it holds
    got = eng.recommend_per_row(seq, 20, np.sort(w_items, axis=1), N)
    ref = eng.recommend(seq, 20, N, dtype="f32")
    assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes()


# ------------------------------------------------------------------------------------------------ 4. rank_targets_per_row
@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_rank_targets_per_row_is_the_count_on_the_logits(i, exclude):
    eng, seq, pos, lg, N = _case(i)
    listed = unlisted = seen_t = 0
    for C in WIDTHS:
        lists = _lists(i, C, 1)
        sets = _sets(lists, N)
        got = eng.rank_targets_per_row(seq, pos, N, lists, exclude_seen=exclude)
        assert got.dtype == np.int32 and got.shape == (seq.shape[0],)
        assert np.array_equal(got, oracle_ranks_rows(lg, pos, sets, seq, exclude)), C
        for b in range(len(sets)):
            inl = pos[b] in sets[b]
            listed, unlisted, seen_t = listed + inl, unlisted + (not inl), seen_t + (pos[b] in seq[b])
    assert listed and unlisted and seen_t                          # a target in its list, one outside it, one among the seen ids
    eng.check_status()


@pytest.mark.parametrize("i", IDS)
def test_rank_over_all_ids_and_over_a_shared_list_equal_the_existing_ranks(i):
    eng, seq, pos, lg, N = _case(i)
    B = seq.shape[0]
    full = np.broadcast_to(np.arange(1, N + 1, dtype=np.int32), (B, N))
    assert np.array_equal(eng.rank_targets_per_row(seq, pos, N, full), eng.rank_targets(seq, pos, N, dtype="f32"))
    shared = np.unique(np.random.RandomState(50 + i).randint(1, eng.item_num + 1, size=max(N // 3, 1)))
    for exclude in (False, True):
        got = eng.rank_targets_per_row(seq, pos, N, np.broadcast_to(shared, (B, len(shared))), exclude_seen=exclude)
        assert np.array_equal(got, eng.rank_targets_among(seq, pos, N, shared, exclude_seen=exclude))


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", IDS)
def test_the_rank_of_a_recommended_item_is_its_column(i, exclude):
    eng, seq, pos, lg, N = _case(i)
    lists = _lists(i, 129, 2)
    items, _ = eng.recommend_per_row(seq, 20, lists, N, exclude_seen=exclude)
    assert (items[:, 0] > 0).any()
    for j in (0, 7, 19):
        tgt = np.where(items[:, j] > 0, items[:, j], 1).astype(np.int32)
        rk = eng.rank_targets_per_row(seq, tgt, N, lists, exclude_seen=exclude)
        assert (rk[items[:, j] > 0] == j).all(), j


@pytest.mark.parametrize("exclude", [False, True])
def test_planted_ties_are_ordered_by_ascending_id(exclude):
    item_num, T, H, L, heads, B, N = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    emb = eng.param("emb")
    tied = [40, 333, 601]
    for j in tied[1:]:
        emb[j] = emb[tied[0]]                                      # one table row on three ids, before the logits are taken
    eng.refresh_shadow()
    lg = eng.logits(seq, N).cpu().numpy()
    assert all(len(set(_bits(lg[b, np.array(tied) - 1]).tolist())) == 1 for b in range(B))
    rs = np.random.RandomState(8)
    lists = np.stack([rs.permutation(np.concatenate([rs.choice(N, size=90, replace=False) + 1, tied])) for _ in range(B)])
    sets = _sets(lists, N)
    for t in tied:
        pos = np.full(B, t, dtype=np.int32)
        got = eng.rank_targets_per_row(seq, pos, N, lists, exclude_seen=exclude)
        assert np.array_equal(got, oracle_ranks_rows(lg, pos, sets, seq, exclude))
    r = [eng.rank_targets_per_row(seq, np.full(B, t, dtype=np.int32), N, lists) for t in tied]
    assert (r[1] == r[0] + 1).all() and (r[2] == r[0] + 2).all()
    _assert_same(eng.recommend_per_row(seq, 64, lists, N, exclude_seen=exclude), _reference_rows(lg, sets, seq, 64, exclude))
    s = eng.score_items(seq, np.tile(np.array(tied), (B, 1)), N)
    assert (_bits(s)[:, 0] == _bits(s)[:, 1]).all() and (_bits(s)[:, 0] == _bits(s)[:, 2]).all()


# ------------------------------------------------------------------------------------------------ 5 + 6. the operators, malformed lists
def _dev(x, dt):
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=dt)).to("cuda")


@pytest.mark.parametrize("i", [0, 2])
def test_the_three_operators_equal_the_engine_calls(i):
    import ader_amd.ops  # noqa: F401
    from ader_amd.engine.infer import row_candidate_ids
    eng, seq, pos, lg, N = _case(i)
    rep, emb = eng.encode(seq), eng.param("emb")
    seq_d = _dev(seq, np.int32)
    for C in (0, 17, 129):
        raw = _lists(i, C, 3)
        got = torch.ops.ader.score_items(rep, emb, _dev(raw, np.int32), N)
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(eng.score_items(seq, raw, N)))
        ids = _dev(row_candidate_ids(raw, N, eng.item_num), np.int32)
        for exclude in (False, True):
            sn = seq_d if exclude else None
            items, scores = torch.ops.ader.topk_items_rows(rep, emb, ids, sn, N, 20)
            _assert_same((items.cpu().numpy(), scores.cpu().numpy()), eng.recommend_per_row(seq, 20, raw, N, exclude_seen=exclude))
            rk = torch.ops.ader.rank_of_target_rows(rep, emb, _dev(pos, np.int32), ids, sn, N)
            assert np.array_equal(rk.cpu().numpy(), eng.rank_targets_per_row(seq, pos, N, raw, exclude_seen=exclude))
    # (the fake-tensor trace of the three operators: tests/test_rowlist_host.py, as the other topk operators')


def test_malformed_rows_set_the_status_and_the_next_call_is_correct():
    import ader_amd.ops  # noqa: F401
    from ader_amd import _lib
    ADER_ST_BAD_CAND = 4                                           # csrc/common.h
    eng, seq, pos, lg, N = _case(0)
    B = seq.shape[0]
    rep, emb = eng.encode(seq), eng.param("emb")
    tgt = _dev(pos, np.int32)
    good = np.zeros((B, 100), dtype=np.int32)
    for b in range(B):
        good[b, :60 + b % 40] = np.arange(5 + b, 5 + b + 3 * (60 + b % 40), 3)      # every id inside [1, N]: nothing here can leave the table
    assert good.max() <= N
    bads = []
    for how in ("descending pair", "duplicate", "id after a 0"):
        bad = good.copy()
        if how == "descending pair":
            bad[B - 1, [70, 71]] = bad[B - 1, [71, 70]]
        elif how == "duplicate":
            bad[10, 64] = bad[10, 63]
            assert bad[10, 64] > 0
        else:
            bad[5, 99] = 7
            assert bad[5, 98] == 0
        assert bad.min() >= 0 and bad.max() <= N
        bads.append((how, bad))
    ref = _reference_rows(lg, _sets(good.astype(np.int64), N), seq, 20, False)
    for how, bad in bads:
        with pytest.raises(RuntimeError, match="ascending"):
            torch.ops.ader.topk_items_rows(rep, emb, _dev(bad, np.int32), None, N, 20)
        with pytest.raises(RuntimeError, match="ascending"):
            torch.ops.ader.rank_of_target_rows(rep, emb, tgt, _dev(bad, np.int32), None, N)
        items, scores = torch.ops.ader.topk_items_rows(rep, emb, _dev(good, np.int32), None, N, 20)
        _assert_same((items.cpu().numpy(), scores.cpu().numpy()), ref, how)
        # the launcher itself: the bit of the status word, and only that
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        Bp = (B + 63) // 64 * 64
        ncol = torch.zeros(Bp, dtype=torch.int32, device="cuda")
        ncol[:B] = N
        tl, rk = torch.zeros(Bp, device="cuda"), torch.zeros(Bp, dtype=torch.int32, device="cuda")
        tg = torch.ones(Bp, dtype=torch.int32, device="cuda")
        bad_d = _dev(bad, np.int32)
        _lib.call("ader_rank_targets_rows", _lib.ptr(rep), _lib.ptr(emb), B, Bp, eng.H, N, _lib.ptr(tg), _lib.ptr(ncol), _lib.ptr(bad_d),
                  100, 100, None, 0, _lib.ptr(tl), _lib.ptr(rk), _lib.ptr(status), torch.cuda.current_stream().cuda_stream)
        assert int(status.item()) == ADER_ST_BAD_CAND, how
    # score_items takes any order: the same matrices are plain inputs there
    for how, bad in bads:
        got = torch.ops.ader.score_items(rep, emb, _dev(bad, np.int32), N).cpu().numpy()
        ok = bad >= 1
        assert np.array_equal(_bits(got[ok]), _bits(lg[np.nonzero(ok)[0], bad[ok] - 1])) and np.isneginf(got[~ok]).all()
    assert np.array_equal(eng.rank_targets_per_row(seq, pos, N, good), oracle_ranks_rows(lg, pos, _sets(good.astype(np.int64), N), seq, False))
    eng.check_status()


def test_launcher_errors_return_minus_two_and_c_zero_is_legal():
    from ader_amd import _lib
    eng, seq, pos, lg, N = _case(2)
    dev, H = eng.device, eng.H
    st = torch.cuda.current_stream().cuda_stream
    ids = torch.ones(64, 8, dtype=torch.int32, device=dev)
    rep = torch.zeros(64, H, device=dev)
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    sc = torch.full((64, 8), 3.0, device=dev)
    part = torch.zeros(64 * 64 * 2, dtype=torch.int64, device=dev)
    items, scores = torch.full((64, 5), 9, dtype=torch.int32, device=dev), torch.zeros(64, 5, device=dev)
    tg, tl, rk = torch.ones(64, dtype=torch.int32, device=dev), torch.zeros(64, device=dev), torch.full((64,), 7, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    for i_, ld, C in ((p(ids), 8, -1), (p(ids), 4, 8), (None, 8, 8)):
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_score_items", p(rep), eng._pp["emb"], 64, H, N, None, i_, ld, C, p(sc), 8, st)
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_topk_items_rows", p(rep), eng._pp["emb"], 64, 64, H, N, p(ncol), i_, ld, C, None, 0, 5, p(part), p(items),
                      p(scores), p(status), st)
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_rank_targets_rows", p(rep), eng._pp["emb"], 64, 64, H, N, p(tg), p(ncol), i_, ld, C, None, 0, p(tl), p(rk),
                      p(status), st)
    with pytest.raises(_lib.AderHipError, match="code -2"):
        _lib.call("ader_topk_items_rows", p(rep), eng._pp["emb"], 64, 64, H, N, p(ncol), p(ids), 8, 8, None, 0,
                  _lib.call("ader_topk_kmax") + 1, p(part), p(items), p(scores), p(status), st)
    assert int(status.item()) == 0 and (rk == 7).all() and (sc == 3.0).all() and (items == 9).all()      # nothing was enqueued
    _lib.call("ader_score_items", p(rep), eng._pp["emb"], 64, H, N, None, None, 0, 0, p(sc), 8, st)
    _lib.call("ader_topk_items_rows", p(rep), eng._pp["emb"], 64, 64, H, N, p(ncol), None, 0, 0, None, 0, 5, p(part), p(items), p(scores),
              p(status), st)
    _lib.call("ader_rank_targets_rows", p(rep), eng._pp["emb"], 64, 64, H, N, p(tg), p(ncol), None, 0, 0, None, 0, p(tl), p(rk), p(status), st)
    assert (sc == 3.0).all() and not items.any() and torch.isneginf(scores).all() and not rk.any() and int(status.item()) == 0
    # ... and through the engine
    e = np.zeros((seq.shape[0], 0), dtype=np.int32)
    assert eng.score_items(seq, e, N).shape == (seq.shape[0], 0)
    it, s_ = eng.recommend_per_row(seq, 5, e, N)
    assert not it.any() and np.isneginf(s_).all() and not eng.rank_targets_per_row(seq, pos, N, e).any()


def test_model_forwarders():
    from ader_amd.main import build_parser
    from ader_amd.model import Ader
    eng, seq, pos, lg, N = _case(2)
    args = build_parser().parse_args(["--hidden_units", "12", "--maxlen", "8", "--num_blocks", "1"])
    model = Ader(64, args)
    lists = [[9, 2, 30, 2], [], [5]]
    a, b = model.recommend_per_row(seq, 3, lists, N, True), model.engine.recommend_per_row(seq, 3, lists, N, exclude_seen=True)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.array_equal(model.rank_targets_per_row(seq, pos, N, lists, True),
                          model.engine.rank_targets_per_row(seq, pos, N, lists, exclude_seen=True))
    items = np.array([[9, 2, 0], [1, 1, 64], [33, 34, -1]])
    assert np.array_equal(_bits(model.score_items(seq, items, N)), _bits(model.engine.score_items(seq, items, N)))
    for bad in ([[1.5]], [[1, 65]], np.array([1, 2])):
        with pytest.raises(RuntimeError):
            model.recommend_per_row(seq, 3, bad, N)
    with pytest.raises(RuntimeError):
        model.recommend_per_row(seq, 3, [[1], [2]], N)             # one list per session


# ------------------------------------------------------------------------------------------------ 7. sampled-negative evaluation
def test_evaluator_with_negatives_equals_the_ranks_computed_from_the_logits(capsys):
    import random

    from ader_amd.data import Evaluator, recall_mrr, sample_negatives
    from ader_amd.main import build_parser
    from ader_amd.model import Ader
    item_num, T, H, L, heads, B, N = SHAPES[1]
    rs = np.random.RandomState(4)
    sessions = [[int(x) for x in rs.randint(1, N + 1, size=int(rs.randint(2, 12)))] for _ in range(200)]
    args = build_parser().parse_args(["--hidden_units", str(H), "--maxlen", str(T), "--num_blocks", str(L), "--num_heads", str(heads)])
    model = Ader(item_num, args)
    random.seed(9)
    plain = Evaluator(sessions, False, T, 64, N, "test", model, None)
    plain_info = plain.evaluate(2)
    plain_out = capsys.readouterr().out
    random.seed(9)
    ev = Evaluator(sessions, False, T, 64, N, "test", model, None, negatives=100, neg_seed=5)
    info = ev.evaluate(2)
    assert capsys.readouterr().out == plain_out and info == plain_info and ev.ranks == plain.ranks
    random.seed(9)
    smp = Evaluator(sessions, False, T, 64, N, "test", model, None).evaluate_sampler
    batches = [smp.next_batch() for _ in range(smp.batch_num())]
    seq = np.concatenate([s for s, p in batches if len(p)])
    pos = np.concatenate([p for s, p in batches if len(p)])
    assert len(pos) == len(ev.ranks_sampled) > 64
    neg = sample_negatives(seq, pos, N, 100, 5)
    lg = model.engine.logits(seq, N).cpu().numpy()
    want = oracle_ranks_rows(lg, pos, list(neg), seq, False)
    assert ev.ranks_sampled == want.tolist() and max(ev.ranks_sampled) <= 100
    assert (np.asarray(ev.ranks_sampled) <= np.asarray(ev.ranks)).all()      # fewer items ahead of the target, never more
    assert ev.results_sampled() == recall_mrr(want)
    assert "among the target and 100 sampled unseen items" in ev.display_sampled(2)


def test_driver_eval_negatives_adds_a_line_and_summary_keys_and_changes_nothing_else(capsys):
    """One period, one epoch of the finetune baseline with and without --eval_negatives 50, same seed: with it the test line is followed by
    the sampled line and the summary entry gains the *_sampled keys; everything else printed is the run without the flag, byte for byte
    (the wall-clock line apart)."""
    import tempfile

    from ader_amd import main as M
    outs, texts, prints = [], [], []
    for extra in ([], ["--eval_negatives", "50"]):
        with tempfile.TemporaryDirectory() as d:
            args = M.build_parser().parse_args(["--dataset", "DIGINETICA", "--max_periods", "1", "--num_epochs", "1", "--finetune", "True",
                                                "--results_root", d] + extra)
            outs.append(M.run(args))
            texts.append(open(os.path.join(d, "DIGINETICA-ADER", "Training_logs.txt")).read().splitlines())
        prints.append([l for l in capsys.readouterr().out.splitlines() if not l.startswith("Total time: ")])
    (p0,), (p1,) = outs[0]["periods"], outs[1]["periods"]
    sampled = [l for l in prints[1] if "sampled unseen items" in l]
    assert len(sampled) == 1 and not [l for l in prints[0] if "sampled" in l]
    assert [l for l in prints[1] if l is not sampled[0]] == prints[0] and len(prints[0]) > 3
    i = prints[1].index(sampled[0])
    assert prints[1][i - 1].startswith("epoch:1, test (MRR@20: ")
    assert sampled[0] == ("epoch:1, test among the target and 50 sampled unseen items (MRR@20: %.4f, RECALL@20: %.4f, MRR@10: %.4f, "
                          "RECALL@10: %.4f)" % (p1["mrr20_sampled"], p1["recall20_sampled"], p1["mrr10_sampled"], p1["recall10_sampled"]))
    assert sampled[0] in texts[1] and not [l for l in texts[0] if "sampled unseen" in l]
    new = {"sampled_negatives", "mrr20_sampled", "recall20_sampled", "mrr10_sampled", "recall10_sampled"}
    assert set(p1) == set(p0) | new and not new & set(p0) and p1["sampled_negatives"] == 50
    assert {k: p1[k] for k in p0} == p0
    for k in ("mrr20", "recall20", "mrr10", "recall10"):
        assert 0.0 < p1[k] <= p1[k + "_sampled"] <= 1.0
    assert outs[0]["average"] == outs[1]["average"]
