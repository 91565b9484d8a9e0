"""Top-K recommendation on the bf16 matrix cores (Engine.recommend(dtype="x3"), torch.ops.ader.topk_items_x3, ader_topk_items_x3): an x3
filter that keeps a superset of every row's top-k, then the exact recheck of the kept pairs.  The contract is byte equality with the
exact-f32 path (dtype="f32": k_topk_tile + k_topk_merge) -- items, order, float32 score bits, ties, item 0 / -inf padding -- for every
input; rows whose kept set outgrows k + band keys are reported in the status word and answered by the f32 kernels."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _kmax():
    from ader_amd._lib import call
    return call("ader_topk_x3_kmax")


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
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.int32), np.ascontiguousarray(ref[1]).view(np.int32))


def _assert_clean(eng, rows):
    """No row left the x3 path, and the observed x3 error stays inside half the band (the bound the rank tests hold)."""
    st = eng.last_topk_stats
    assert st["rows"] == rows and st["overflowed_rows"] == 0 and st["fallback_chunks"] == 0, st
    assert st["max_err_over_delta"] <= 0.5, st


# item_num, T, H, L, heads, B, N, k (None: ader_topk_x3_kmax(); "min64": min(64, that))
SHAPES = [(700, 50, 150, 2, 1, 70, 650, 20),          # N no multiple of 32, B under one 128-row chunk
          (1000, 50, 150, 2, 3, 130, 777, None),      # two chunks, k at the x3 limit
          (64, 8, 12, 1, 1, 3, 33, "min64"),          # k > N: padding, more of it with exclusion
          (64, 8, 12, 1, 1, 1, 1, 1),                 # N = 1, k = 1
          (2000, 20, 150, 1, 1, 1030, 1999, 5),       # over MAX_ROWS: two engine chunks
          (40000, 20, 64, 1, 1, 70, 40000, 20)]       # a workgroup walks several blocks


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions and the f32 path's answers (exclude off / on) of SHAPES[i]: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N, k = SHAPES[i]
    k = _kmax() if k is None else min(64, _kmax()) if k == "min64" else k
    eng = _engine(item_num, T, H, L, heads)
    seq = _seqs(np.random.RandomState(6 + i), B, T, N)
    seq.setflags(write=False)
    ref = {ex: eng.recommend(seq, k, N, exclude_seen=ex, dtype="f32") for ex in (False, True)}
    return eng, seq, ref, N, k


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_engine_x3_equals_f32_bytewise(i, exclude):
    from ader_amd._lib import call
    eng, seq, ref, N, k = _case(i)
    got = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="x3")
    _assert_same(got, ref[exclude])
    _assert_clean(eng, seq.shape[0])
    if i == 0:                                   # a reference that does not go through ader_topk_items
        _assert_same(got, _reference(eng.logits(seq, N).cpu().numpy(), seq, k, exclude))
    if i == 5:
        B = min(seq.shape[0], eng.MAX_ROWS)
        assert (N + 31) // 32 > call("ader_topk_x3_ranges", N, (B + 127) // 128 * 128)       # thresholds carry over from block to block


def test_engine_option_is_the_default_of_dtype_none_and_unsupported_shapes_take_f32():
    eng, seq, ref, N, k = _case(0)
    assert eng.topk_dtype == "f32"
    eng.last_topk_stats = None
    _assert_same(eng.recommend(seq, k, N), ref[False])
    assert eng.last_topk_stats is None                                           # the f32 path leaves no x3 statistics
    eng.topk_dtype = "x3"
    try:
        _assert_same(eng.recommend(seq, k, N), ref[False])
        _assert_clean(eng, seq.shape[0])
        if _kmax() < 64:                                                          # k beyond the x3 limit: the f32 kernels, silently
            eng.last_topk_stats = None
            _assert_same(eng.recommend(seq, 64, N), eng.recommend(seq, 64, N, dtype="f32"))
            assert eng.last_topk_stats is None
    finally:
        eng.topk_dtype = "f32"
    e10 = _engine(64, 8, 10, 1, 1, topk_dtype="x3")                              # H mod 8 = 2: outside k_lx3t's hidden sizes
    s10 = _seqs(np.random.RandomState(1), 5, 8, 64)
    _assert_same(e10.recommend(s10, 5), e10.recommend(s10, 5, dtype="f32"))
    assert e10.last_topk_stats is None
    for bad in ("bf16", "X3"):
        with pytest.raises(RuntimeError, match="topk_dtype"):
            eng.recommend(seq, k, N, dtype=bad)
    for bad_band in (-1, 17):
        with pytest.raises(RuntimeError, match="band"):
            eng.recommend(seq, k, N, dtype="x3", band=bad_band)


def _planted(copies_of, ids, ulps=None):
    """SHAPES[0]'s engine (the same seed: the same parameters as the shared one) with table row `copies_of` copied to `ids`; ulps: per
    copy, channel 0 moved by that many ulp."""
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    emb = eng.param("emb")
    for j, n in enumerate(ids):
        emb[n] = emb[copies_of]
        if ulps is not None:
            x = emb[n, 0].item()
            emb[n, 0] = float(np.float32(x) + np.float32(ulps[j]) * np.spacing(np.float32(x)))
    eng.refresh_shadow()
    return eng


def test_planted_ties_lead_in_ascending_id():
    eng0, seq, ref, N, k = _case(0)
    t = int(ref[False][0][0, 0])
    tied = sorted({t, 3, 200, N - 2})            # blocks 0, 6 and 20 of 21, each in a range of its own
    eng = _planted(t, tied)
    got = eng.recommend(seq, k, N, dtype="x3")
    _assert_same(got, eng.recommend(seq, k, N, dtype="f32"))
    _assert_clean(eng, seq.shape[0])
    assert list(got[0][0, :len(tied)]) == tied and len(set(got[1][0, :len(tied)].tolist())) == 1


def test_planted_near_ties_straddle_rank_k():
    eng0, seq, ref, N, k = _case(0)
    kth, beyond = int(ref[False][0][0, k - 1]), [int(x) for x in ref[False][0][0]]
    ids = [n for n in (5, 77, 333, N - 1) if n not in beyond]
    eng = _planted(kth, ids, ulps=[1, -2, 3, -4][:len(ids)])
    got = eng.recommend(seq, k, N, dtype="x3")
    want = eng.recommend(seq, k, N, dtype="f32")
    _assert_same(got, want)
    _assert_clean(eng, seq.shape[0])
    inside = set(ids + [kth]) & set(want[0][0].tolist())            # the near-tied items sit at ranks k .. k + len(ids) of row 0
    assert 1 <= len(inside) <= len(ids)


def test_band_zero_hands_tied_rows_to_the_f32_kernels():
    eng0, seq, ref, N, k = _case(0)
    kth, top = int(ref[False][0][0, k - 1]), set(ref[False][0][0].tolist())
    other = next(n for n in range(1, N + 1) if n not in top)
    eng = _planted(kth, [other])                 # row 0: two equal scores across rank k -> k + 1 keys kept, over k + 0
    for exclude in (False, True):
        got = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="x3", band=0)
        _assert_same(got, eng.recommend(seq, k, N, exclude_seen=exclude, dtype="f32"))
        st = eng.last_topk_stats
        assert st["overflowed_rows"] >= (0 if exclude else 1) and st["fallback_chunks"] == (1 if st["overflowed_rows"] else 0), st


# ---------------------------------------------------------------------------------------------- operator level
def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to("cuda")


def _op(rep, emb, seen, N, k, x3=True):
    import ader_amd.ops  # noqa: F401
    fn = torch.ops.ader.topk_items_x3 if x3 else torch.ops.ader.topk_items
    items, scores = fn(_dev(rep), _dev(emb), _dev(seen), N, k)
    return items.cpu().numpy(), scores.cpu().numpy()


def _raw(rep, emb, seen, N, k, band=16, H=None, Bp=None, item_num=None, check=True):
    """ader_topk_items_x3 itself, no fallback: (items, scores, status [B], diag [3]) or the return code (check=False)."""
    from ader_amd import _lib
    B, H = rep.shape[0], rep.shape[1] if H is None else H
    Bp = (B + 127) // 128 * 128 if Bp is None else Bp
    Bq = (Bp + 127) // 128 * 128
    dev = torch.device("cuda")
    r, e, s = _dev(rep), _dev(emb), _dev(seen)
    ncol = torch.zeros(Bq, dtype=torch.int32, device=dev)
    ncol[:B] = N
    hi, lo = (torch.zeros(Bq * 168, dtype=torch.bfloat16, device=dev) for _ in range(2))
    delta, emax = torch.zeros(Bq, device=dev), torch.zeros(1, device=dev)
    part3 = torch.zeros(max(1, _lib.call("ader_topk_x3_ranges", max(N, 1), Bq)) * Bq * (max(k, 1) + max(band, 0)), dtype=torch.int64, device=dev)
    status, diag = torch.zeros(Bq, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
    items, scores = torch.zeros(B, max(k, 1), dtype=torch.int32, device=dev), torch.zeros(B, max(k, 1), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    inum = emb.shape[0] - 1 if item_num is None else item_num
    args = (_lib.ptr(r), _lib.ptr(e), inum, B, Bp, H, N, _lib.ptr(ncol), _lib.ptr(s), seen.shape[1] if seen is not None else 0, k, band,
            _lib.ptr(hi), _lib.ptr(lo), _lib.ptr(delta), _lib.ptr(emax), _lib.ptr(part3), _lib.ptr(status), _lib.ptr(diag),
            _lib.ptr(items), _lib.ptr(scores), st)
    if not check:
        return _lib.load().ader_topk_items_x3(*args)
    _lib.call("ader_rank_emax", _lib.ptr(e), inum, H, N, _lib.ptr(emax), st)
    _lib.call("ader_topk_items_x3", *args)
    return items.cpu().numpy(), scores.cpu().numpy(), status[:B].cpu().numpy(), diag.cpu().numpy()


def _assert_rows(raw, ref, expect_over):
    """The launcher's own output: rows with status 0 are the reference's bytes, and exactly the expected rows carry a status."""
    items, scores, status, diag = raw
    ok = status == 0
    assert np.array_equal(~ok, expect_over), (np.nonzero(~ok)[0], np.nonzero(expect_over)[0])
    _assert_same((items[ok], scores[ok]), (ref[0][ok], ref[1][ok]))
    assert diag[1] == int(expect_over.sum()) and diag[2:3].view(np.float32)[0] <= 0.5


def _int_operands(kind, B, N, H, rs):
    """Small-integer operands: every product and partial sum is an exact float32, so the int64 product is the expected score."""
    rep = rs.randint(-3, 4, size=(B, H)).astype(np.float32)
    emb = rs.randint(-3, 4, size=(N + 60, H)).astype(np.float32)
    if kind != "random":
        emb[:] = 0
        rep[:, 0] = 1 + np.arange(B) % 3
        emb[:, 0] = {"increasing": np.arange(N + 60), "decreasing": -np.arange(N + 60), "constant": np.full(N + 60, 2)}[kind]
    return rep, emb


def _int_scores(rep, emb, N):
    return (rep.astype(np.int64) @ emb[1:N + 1].astype(np.int64).T).astype(np.float32)        # exact: |score| < 2^24


@pytest.mark.parametrize("kind", ["increasing", "decreasing", "constant", "random"])
def test_integer_operands_equal_f32_and_the_int64_product(kind):
    """increasing: every item beats the row's edge, so every block appends 32 keys per row and compacts -- the worst case of the buffer
    invariant; decreasing: nothing passes after the first compaction; constant: the whole catalog ties, every row with more than k + band
    items overflows and comes back through the f32 kernels; random: many equal integer scores, rows overflow where they tie across rank k."""
    rs = np.random.RandomState(3)
    for N in (31, 32, 33, 4097):
        for B in (1, 128, 129):
            rep, emb = _int_operands(kind, B, N, 12, rs)
            want = _int_scores(rep, emb, N)
            for k in (5, _kmax()):
                ref = _op(rep, emb, None, N, k, x3=False)
                _assert_same(ref, _reference(want, None, k, False))
                _assert_same(_op(rep, emb, None, N, k), ref)
                if kind == "constant":
                    _assert_rows(_raw(rep, emb, None, N, k), ref, np.full(B, N > k + 16))
                elif kind != "random":
                    _assert_rows(_raw(rep, emb, None, N, k), ref, np.zeros(B, dtype=bool))


@pytest.mark.parametrize("kind", ["increasing", "random"])
def test_seen_lists_with_duplicates_zeros_and_ids_above_n(kind):
    rs = np.random.RandomState(4)
    for N in (33, 4097):
        for B in (1, 129):
            rep, emb = _int_operands(kind, B, N, 12, rs)
            seen = rs.randint(N - 40, N + 50, size=(B, 9)).astype(np.int32)         # the best ids of "increasing", some above N
            seen[:, 1], seen[:, 2], seen[:, 3] = seen[:, 0], 0, rs.randint(1, 20, size=B)
            seen[seen < 0] = 0
            assert (seen > N).any() and (seen == 0).any()
            ref = _op(rep, emb, seen, N, 20, x3=False)
            _assert_same(ref, _reference(_int_scores(rep, emb, N), seen, 20, True))
            _assert_same(_op(rep, emb, seen, N, 20), ref)
    rep, emb = _int_operands("constant", 3, 33, 12, rs)                              # everything seen: nothing to return
    seen = np.tile(np.arange(1, 34, dtype=np.int32), (3, 1))
    items, scores = _op(rep, emb, seen, 33, 7)
    assert (items == 0).all() and np.isneginf(scores).all()


def _gauss(B, N, H, seed, scale):
    rs = np.random.RandomState(seed)
    rep = rs.standard_normal((B, H)).astype(np.float32)
    return rep, (rs.standard_normal((N + 1, H)) * scale).astype(np.float32), rs


@pytest.mark.parametrize("B,N,H,seed,scale", [(130, 777, 150, 5, 0.05), (70, 40000, 150, 7, 0.05), (130, 4097, 12, 9, 1.0),
                                              (257, 100000, 64, 3, 0.05)])
def test_gaussian_operands_do_not_overflow(B, N, H, seed, scale):
    """tests/test_topk_x3_host.py holds these operands' band populations at or below half the band: no row may leave the x3 path."""
    rep, emb, _ = _gauss(B, N, H, seed, scale)
    for k in (20, _kmax()):
        ref = _op(rep, emb, None, N, k, x3=False)
        _assert_rows(_raw(rep, emb, None, N, k), ref, np.zeros(B, dtype=bool))


def test_crowded_band_overflows_those_rows_only():
    """band + 5 copies of a row's k-th best item: that row keeps k - 1 + band + 6 equal-or-better keys and overflows; the rows for which
    the copies lie far below their k-th best (checked in float64, in units of the band width) must not."""
    B, N, H, k, band = 40, 4097, 64, 20, 16
    rep, emb, rs = _gauss(B, N, H, 21, 0.05)
    crowded = [3, 17]
    for b in crowded:
        s = rep[b].astype(np.float64) @ emb[1:].astype(np.float64).T
        kth = int(np.argsort(-s, kind="stable")[k - 1]) + 1
        for n in rs.choice(np.arange(1, N + 1), size=band + 5, replace=False):
            if n != kth:
                emb[n] = emb[kth]
    s64 = rep.astype(np.float64) @ emb[1:].astype(np.float64).T
    d = 2.0 ** -13 * np.linalg.norm(rep.astype(np.float64), axis=1) * np.linalg.norm(emb[1:].astype(np.float64), axis=1).max()
    kth = -np.sort(-s64, axis=1)[:, k - 1]
    near = ((s64 >= (kth - 3 * d)[:, None]).sum(1) - k)              # items at or within 3 band widths below the k-th best
    expect = np.zeros(B, dtype=bool)
    expect[crowded] = True
    assert (near[crowded] >= band + 3).all() and (near[~expect] <= band // 2).all()          # the premise: unambiguous either way
    ref = _op(rep, emb, None, N, k, x3=False)
    _assert_rows(_raw(rep, emb, None, N, k, band=band), ref, expect)
    _assert_same(_op(rep, emb, None, N, k), ref)


def test_zero_rep_row_and_non_finite_values():
    B, N, H, k = 9, 300, 64, 20
    rep, emb, _ = _gauss(B, N, H, 2, 0.05)
    rep[2] = 0.0                                                     # every score 0: the whole catalog ties
    ref = _op(rep, emb, None, N, k, x3=False)
    expect = np.zeros(B, dtype=bool)
    expect[2] = True
    _assert_rows(_raw(rep, emb, None, N, k), ref, expect)
    _assert_same(_op(rep, emb, None, N, k), ref)
    assert list(ref[0][2]) == list(range(1, k + 1))
    rep[4, 7], emb[50, 3], emb[60, 1] = np.inf, np.nan, -np.inf
    _assert_same(_op(rep, emb, None, N, k), _op(rep, emb, None, N, k, x3=False))


@pytest.mark.parametrize("with_seen", [False, True])
def test_rows_are_independent_and_calls_repeat(with_seen):
    B, N, H, k = 130, 777, 150, 20
    rep, emb, rs = _gauss(B, N, H, 5, 0.05)
    seen = rs.randint(0, N + 1, size=(B, 11)).astype(np.int32) if with_seen else None
    full = _op(rep, emb, seen, N, k)
    again = _op(rep, emb, seen, N, k)
    assert full[0].tobytes() == again[0].tobytes() and full[1].tobytes() == again[1].tobytes()
    for b in (0, 70, 129):                       # first chunk, second chunk
        one = _op(rep[b:b + 1].copy(), emb, None if seen is None else seen[b:b + 1].copy(), N, k)
        assert one[0].tobytes() == full[0][b:b + 1].tobytes() and one[1].tobytes() == full[1][b:b + 1].tobytes()


def test_errors():
    kmax = _kmax()
    rep, emb, _ = _gauss(5, 100, 64, 1, 0.05)
    import ader_amd.ops  # noqa: F401
    for bad_k in (0, kmax + 1):
        assert _raw(rep, emb, None, 100, bad_k, check=False) == -2
        with pytest.raises(RuntimeError):
            torch.ops.ader.topk_items_x3(_dev(rep), _dev(emb), None, 100, bad_k)
    for bad_n in (0, 101):
        assert _raw(rep, emb, None, bad_n, 5, check=False) == -2
        with pytest.raises(RuntimeError):
            torch.ops.ader.topk_items_x3(_dev(rep), _dev(emb), None, bad_n, 5)
    assert _raw(rep, emb, None, 100, 5, band=-1, check=False) == -2
    assert _raw(rep, emb, None, 100, 5, Bp=64, check=False) == -2                    # Bp % 128 != 0
    assert _raw(rep, emb, None, 100, 5, H=10, check=False) == -2                     # H mod 8 = 2
    assert _raw(rep, emb, None, 100, 5, item_num=2 ** 31 // (64 * 4), check=False) == -2      # a table of 2^31 bytes: 32-bit block offsets
    r10, e10, _ = _gauss(5, 100, 10, 1, 0.05)
    with pytest.raises(RuntimeError, match="H must be"):
        torch.ops.ader.topk_items_x3(_dev(r10), _dev(e10), None, 100, 5)
