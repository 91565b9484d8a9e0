"""Exact top-K recommendation fused with the catalog logits (Engine.recommend, torch.ops.ader.topk_items, ader_topk_items).  The contract
is a pair of equalities against code that is already trusted: (a) items == stable_argsort(-Engine.logits)[:, :k] + 1 with the gathered
device logits as scores, bit for bit; (b) Engine.rank_targets(seq_b, items[b, j]) == j.  Order: (score descending, item id ascending)."""
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


def _seqs(rs, B, T, n_items, full=False):
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = T if full else int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


# item_num, T, H, L, heads, B, N, k
SHAPES = [(700, 50, 150, 2, 1, 70, 650, 20),          # rows over one chunk, N no multiple of 64
          (300, 20, 64, 1, 2, 9, 300, 10),            # small batch, two heads
          (1000, 50, 150, 2, 3, 130, 777, 64),        # three chunks, k at K_MAX
          (64, 8, 12, 1, 1, 3, 33, 64),               # k > N: padding, more of it with exclusion
          (64, 8, 12, 1, 1, 1, 1, 1),                 # N = 1, k = 1
          (2000, 20, 150, 1, 1, 1030, 1999, 5),       # over MAX_ROWS: two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000, 20)]      # a workgroup walks several tiles


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


def _assert_same(got, ref):
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[0].shape == ref[0].shape == got[1].shape
    assert np.array_equal(got[0], ref[0])
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.int32), ref[1].view(np.int32))


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


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_items_are_the_head_of_the_stable_argsort_of_the_device_logits(i, exclude):
    from ader_amd._lib import call
    eng, seq, lg, N, k = _case(i)
    got = eng.recommend(seq, k, N, exclude_seen=exclude)
    _assert_same(got, _reference(lg, seq, k, exclude))
    B = min(seq.shape[0], eng.MAX_ROWS)
    tiles, ranges = (N + 63) // 64, call("ader_topk_ranges", N, (B + 63) // 64 * 64)
    if i == 6:
        assert tiles > ranges           # a workgroup owns several tiles: thresholds carry over, compaction after the first
    if i == 0:
        assert tiles <= ranges          # at most one tile per workgroup, trailing ranges empty


@pytest.mark.parametrize("i", [0, 2])
def test_rank_of_the_jth_item_is_j(i):
    eng, seq, lg, N, k = _case(i)
    items, _ = eng.recommend(seq, k, N)
    assert (items > 0).all()
    ranks = eng.rank_targets(np.repeat(seq, k, axis=0), items.reshape(-1), N, dtype="f32")
    assert np.array_equal(ranks.reshape(-1, k), np.tile(np.arange(k, dtype=np.int32), (seq.shape[0], 1)))


def test_planted_ties_lead_in_ascending_id():
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    t = int(_reference(_case(0)[2], seq, k, False)[0][0, 0])          # (the same seed: the same parameters as the shared engine)
    emb = eng.param("emb")
    tied = sorted({t, 3, 200, N - 2})           # items 3, 200, N-2: tiles 0, 3 and 10 of 11, each in a range of its own
    for j in tied:
        emb[j] = emb[t]
    eng.refresh_shadow()
    lg = eng.logits(seq, N).cpu().numpy()
    got = eng.recommend(seq, k, N)
    _assert_same(got, _reference(lg, seq, k, False))
    assert list(got[0][0, :len(tied)]) == tied and len(set(got[1][0, :len(tied)].tolist())) == 1


@pytest.mark.parametrize("exclude", [False, True])
def test_total_tie_returns_the_first_ids(exclude):
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    emb = eng.param("emb")
    emb[1:N + 1] = emb[1].clone()
    eng.refresh_shadow()
    items, scores = eng.recommend(seq, k, N, exclude_seen=exclude)
    for b in range(B):
        unseen = [n for n in range(1, N + 1) if not (exclude and n in set(seq[b].tolist()))][:k]
        assert list(items[b]) == unseen
    assert (scores == scores[:, :1]).all()
    _assert_same((items, scores), _reference(eng.logits(seq, N).cpu().numpy(), seq, k, exclude))


# ---------------------------------------------------------------------------------------------- operator level, exact integers
def _int_operands(kind, B, N, H, rs):
    """Small-integer operands: every product and partial sum is an exact float32, so the int64 product is the expected score."""
    rep = rs.randint(-3, 4, size=(B, H)).astype(np.float32)
    emb = rs.randint(-3, 4, size=(N + 60, H)).astype(np.float32)
    if kind != "random":
        emb[:] = 0
        rep[:, 0] = 1 + np.arange(B) % 3
        emb[:, 0] = {"increasing": np.arange(N + 60), "decreasing": -np.arange(N + 60), "constant": np.full(N + 60, 2)}[kind]
    return rep, emb


def _op(rep, emb, seen, N, k):
    import ader_amd.ops  # noqa: F401
    dev = torch.device("cuda")
    s = None if seen is None else torch.from_numpy(seen).to(dev)
    items, scores = torch.ops.ader.topk_items(torch.from_numpy(rep).to(dev), torch.from_numpy(emb).to(dev), s, N, k)
    return items.cpu().numpy(), scores.cpu().numpy()


def _int_scores(rep, emb, N):
    return (rep.astype(np.int64) @ emb[1:N + 1].astype(np.int64).T).astype(np.float32)        # exact: |score| < 2^24


@pytest.mark.parametrize("kind", ["increasing", "decreasing", "constant", "random"])
def test_integer_operands_match_int64_product(kind):
    """increasing: every item beats the row's threshold, so every tile appends 64 keys per row and compacts -- the worst case of the
    buffer invariant; decreasing: nothing passes after the first k; constant and random: ties decided by the item id."""
    rs = np.random.RandomState(3)
    for N in (63, 64, 65, 4097):
        for B in (1, 64, 65):
            rep, emb = _int_operands(kind, B, N, 12, rs)
            s = _int_scores(rep, emb, N)
            for k in (5, 64):
                _assert_same(_op(rep, emb, None, N, k), _reference(s, None, k, False))


@pytest.mark.parametrize("kind", ["increasing", "random"])
def test_seen_lists_with_duplicates_zeros_and_ids_above_n(kind):
    rs = np.random.RandomState(4)
    for N in (65, 4097):
        for B in (1, 65):
            rep, emb = _int_operands(kind, B, N, 12, rs)
            seen = rs.randint(N - 40, N + 50, size=(B, 9)).astype(np.int32)         # the best ids of "increasing", some above N
            seen[:, 1], seen[:, 2], seen[:, 3] = seen[:, 0], 0, rs.randint(1, 20, size=B)
            assert (seen > N).any() and (seen == 0).any()
            _assert_same(_op(rep, emb, seen, N, 20), _reference(_int_scores(rep, emb, N), seen, 20, True))
    rep, emb = _int_operands("constant", 3, 33, 12, rs)                              # everything seen: nothing to return
    seen = np.tile(np.arange(1, 34, dtype=np.int32), (3, 1))
    items, scores = _op(rep, emb, seen, 33, 7)
    assert (items == 0).all() and np.isneginf(scores).all()


@pytest.mark.parametrize("with_seen", [False, True])
def test_rows_are_independent_and_calls_repeat(with_seen):
    B, N, H, k = 130, 777, 150, 20
    rs = np.random.RandomState(5)
    rep = rs.standard_normal((B, H)).astype(np.float32)
    emb = (rs.standard_normal((N + 1, H)) * 0.05).astype(np.float32)
    seen = rs.randint(0, N + 1, size=(B, 11)).astype(np.int32) if with_seen else None
    full = _op(rep, emb, seen, N, k)
    again = _op(rep, emb, seen, N, k)
    assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
    for b in (0, 70, 129):                       # first, middle and last chunk
        one = _op(rep[b:b + 1].copy(), emb, None if seen is None else seen[b:b + 1].copy(), N, k)
        assert one[0].tobytes() == full[0][b:b + 1].tobytes() and one[1].tobytes() == full[1][b:b + 1].tobytes()


def test_against_the_float64_oracle():
    """The device logits are within tol = 1e-4 max(1, max |lg_o|) of the oracle's (tests/test_gpu_shim.py), so a returned item may
    trail the oracle's k-th best by at most 2 tol, and no omitted item may lead the worst returned one by more."""
    from oracle import ader_ref_cpu as R
    eng, seq, lg, N, k = _case(1)
    items, _ = eng.recommend(seq, k, N)
    params = {n: v.double() for n, v in eng.export_params().items()}
    rep_o = R.forward_rep(params, seq.astype(np.int64), eng.L, eng.heads, training=False)
    lg_o = R.logits_from_rep(params, rep_o, N).numpy()
    tol = 1e-4 * max(1.0, np.abs(lg_o).max())
    for b in range(seq.shape[0]):
        assert (items[b] > 0).all() and len(set(items[b].tolist())) == k
        mine = lg_o[b, items[b] - 1]
        kth = np.sort(lg_o[b])[-k]
        assert (mine >= kth - 2 * tol).all()
        rest = np.delete(lg_o[b], items[b] - 1)
        assert rest.max() <= mine.min() + 2 * tol


def test_errors():
    from ader_amd import _lib
    eng, seq, lg, N, k = _case(3)
    kmax = _lib.call("ader_topk_kmax")
    assert kmax == 64
    for bad_k in (0, kmax + 1):
        with pytest.raises(RuntimeError):
            eng.recommend(seq, bad_k, N)
    for bad_n in (0, eng.item_num + 1):
        with pytest.raises(RuntimeError):
            eng.recommend(seq, 5, bad_n)
    dev = eng.device
    rep = torch.zeros(64, eng.H, device=dev)
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    part = torch.zeros(_lib.call("ader_topk_ranges", N, 64) * 64 * (kmax + 1), dtype=torch.int64, device=dev)
    items = torch.zeros(64, kmax + 1, dtype=torch.int32, device=dev)
    scores = torch.zeros(64, kmax + 1, device=dev)
    with pytest.raises(_lib.AderHipError, match="code -2"):
        _lib.call("ader_topk_items", _lib.ptr(rep), eng._pp["emb"], 64, 64, eng.H, N, _lib.ptr(ncol), None, 0, kmax + 1, _lib.ptr(part),
                  _lib.ptr(items), _lib.ptr(scores), torch.cuda.current_stream().cuda_stream)
