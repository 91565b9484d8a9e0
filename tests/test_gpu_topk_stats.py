"""Top-K with model probabilities (Engine.recommend_stats / row_stats, torch.ops.ader.topk_items_stats / row_stats, Ader.recommend_probs):
the row's log-sum-exp and entropy over ALL items 1..N out of the top-K walk.  The contract: items / scores are recommend(dtype="f32")'s
bytes; lse / entropy do not depend on exclusion, are the same bits from the fused and the statistics-only kernel and from run to run,
and agree with float64 over the DEVICE float32 logits (Engine.logits) within a few float32 ulp at max(1, |lse|)."""
import functools
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# Tolerances in float32 ulp at max(1, |lse_ref|), 4 x the worst |got - ref64| over SHAPES measured on the MI355X, rounded up to whole
# ulp (profiles/topk_stats.txt; the margin is for other batch sizes and range counts, which reorder the sums), capped at 4 ulp.
# Measured worst: lse 0.593 ulp (shape 2), entropy 0.723 ulp (shape 4).
LSE_TOL_ULP = 3            # ceil(4 x 0.593)
ENT_TOL_ULP = 3            # ceil(4 x 0.723)
assert LSE_TOL_ULP <= 4 and ENT_TOL_ULP <= 4


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
SHAPES = [(700, 50, 150, 2, 1, 70, 650, 20),          # two chunks; N no multiple of 64; at most one tile per range; trailing ranges empty
          (300, 20, 64, 1, 2, 9, 300, 10),            # small batch; H = 64
          (64, 8, 12, 1, 1, 3, 33, 64),               # k > N: padding
          (64, 8, 12, 1, 1, 1, 1, 1),                 # N = 1: lse has the score's bits, entropy == 0.0 exactly
          (2000, 20, 150, 1, 1, 1030, 1999, 5),       # over MAX_ROWS: two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000, 20)]      # several tiles per range: the per-lane state carries across tiles


def _ref64(lg):
    """float64 (lse, entropy) of float32 logits lg [n, N]."""
    s = lg.astype(np.float64)
    m = s.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(axis=1))
    d = s - lse[:, None]
    return lse, -(np.exp(d) * d).sum(axis=1)


def _ulp(lse_ref):
    return np.spacing(np.maximum(1.0, np.abs(lse_ref)).astype(np.float32)).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions, the device logits of SHAPES[i] and their float64 statistics: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N, k = SHAPES[i]
    eng = _engine(item_num, T, H, L, heads)
    seq = _seqs(np.random.RandomState(6 + i), B, T, N)
    lg = eng.logits(seq, N).cpu().numpy()
    ref = _ref64(lg)
    for a in (lg, seq) + ref:
        a.setflags(write=False)
    return eng, seq, lg, N, k, ref


@functools.lru_cache(maxsize=None)
def _fused(i, exclude):
    eng, seq, lg, N, k, ref = _case(i)
    out = eng.recommend_stats(seq, k, N, exclude_seen=exclude)
    for a in out:
        a.setflags(write=False)
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_items_and_scores_are_recommends_bytes(i, exclude):
    from ader_amd._lib import call
    eng, seq, lg, N, k, ref = _case(i)
    items, scores, lse, ent = _fused(i, exclude)
    r_items, r_scores = eng.recommend(seq, k, N, exclude_seen=exclude, dtype="f32")
    assert items.dtype == np.int32 and items.shape == r_items.shape == (seq.shape[0], k) and np.array_equal(items, r_items)
    assert _same_bits(scores, r_scores)
    assert lse.dtype == ent.dtype == np.float32 and lse.shape == ent.shape == (seq.shape[0],)
    B = min(seq.shape[0], eng.MAX_ROWS)
    tiles, ranges = (N + 63) // 64, call("ader_topk_ranges", N, (B + 63) // 64 * 64)
    if i == 5:
        assert tiles > ranges           # a workgroup owns several tiles: the per-lane state carries across them
    if i == 0:
        assert tiles <= ranges          # at most one tile per workgroup, trailing ranges empty: empty partials are merged


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_exclusion_does_not_move_the_normaliser(i):
    a, b = _fused(i, False), _fused(i, True)
    assert _same_bits(a[2], b[2]) and _same_bits(a[3], b[3])
    if i in (0, 1):
        assert not np.array_equal(a[0], b[0])        # (the answers do differ: something was excluded)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_fused_equals_statistics_only_and_calls_repeat(i):
    eng, seq, lg, N, k, ref = _case(i)
    lse, ent = eng.row_stats(seq, N)
    assert _same_bits(lse, _fused(i, False)[2]) and _same_bits(ent, _fused(i, False)[3])
    lse2, ent2 = eng.row_stats(seq, N)
    assert _same_bits(lse, lse2) and _same_bits(ent, ent2)
    again = eng.recommend_stats(seq, k, N, exclude_seen=True)
    for x, y in zip(again, _fused(i, True)):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_against_float64_over_the_device_logits(i):
    eng, seq, lg, N, k, ref = _case(i)
    items, scores, lse, ent = _fused(i, False)
    u = _ulp(ref[0])
    e_lse, e_ent = np.abs(lse.astype(np.float64) - ref[0]) / u, np.abs(ent.astype(np.float64) - ref[1]) / u
    print("shape %d: worst lse error %.3f ulp, worst entropy error %.3f ulp (lse in [%.3f, %.3f])" %
          (i, e_lse.max(), e_ent.max(), ref[0].min(), ref[0].max()))
    assert np.isfinite(lse).all() and np.isfinite(ent).all()
    assert e_lse.max() <= LSE_TOL_ULP and e_ent.max() <= ENT_TOL_ULP
    if i == 3:                                       # N = 1
        assert _same_bits(lse, np.ascontiguousarray(lg[:, 0])) and (ent == 0.0).all()


# ---------------------------------------------------------------------------------------------- planted edges
def test_a_planted_dominant_item_at_the_edges_of_tiles_and_of_the_catalog():
    """One table row = alpha * rep_b makes that item's logit of row b stand >= 30 above every other: lse[b] is then that logit and the
    entropy vanishes, wherever in the walk the item sits (first and last item, both sides of a tile boundary); an item beyond max_item
    counts for nothing.  The item is in no session, so the representations do not move."""
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    edges = [1, 64, 65, N - 1, N]
    seq = np.array(_case(0)[1])
    seq[np.isin(seq, edges + [N + 1])] = 2           # (sessions hold ids <= N: N + 1 is free anyway)
    b = 37
    rep = eng.encode(seq).cpu().numpy()
    lg0 = eng.logits(seq, N).cpu().numpy()
    base = eng.row_stats(seq, N)
    emb = eng.param("emb")
    row = torch.from_numpy((60.0 / float(rep[b] @ rep[b])) * rep[b]).to(emb.device)
    for p in edges + [N + 1]:
        keep = emb[p].clone()
        emb[p] = row
        eng.refresh_shadow()
        lse, ent = eng.row_stats(seq, N)
        f = eng.recommend_stats(seq, k, N)
        assert _same_bits(lse, f[2]) and _same_bits(ent, f[3])
        if p <= N:
            logit = eng.score_items(seq, np.full((B, 1), p, dtype=np.int32), N)[b, 0]      # (the same batch: the same forward)
            assert logit - np.delete(lg0[b], p - 1).max() >= 30.0
            assert f[0][b, 0] == p and f[1][b, 0] == logit
            assert abs(float(lse[b]) - float(logit)) <= LSE_TOL_ULP * float(np.spacing(np.float32(abs(logit))))
            assert 0.0 <= ent[b] < 1e-6
            assert np.isfinite(lse).all() and np.isfinite(ent).all() and (ent >= 0.0).all()
        else:
            assert _same_bits(lse, base[0]) and _same_bits(ent, base[1])      # nothing beyond max_item counts
        emb[p] = keep
    eng.refresh_shadow()
    lse, ent = eng.row_stats(seq, N)
    assert _same_bits(lse, base[0]) and _same_bits(ent, base[1])


def test_a_seen_item_keeps_its_mass():
    """The planted item among row b's seen ids under exclusion: it leaves the answer, not the normaliser.  At the operator level, where
    the seen ids are an argument of their own: planting an item of the row's session would move its representation."""
    import ader_amd.ops  # noqa: F401
    item_num, T, H, L, heads, B, N, k = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = np.array(_case(0)[1])
    b, p = 5, 65
    seq[seq == p] = 2
    rep = eng.encode(seq)
    table = eng.param("emb").detach().clone().contiguous()
    r = rep[b]
    table[p] = (60.0 / float(r @ r)) * r
    seen = torch.from_numpy(np.concatenate([seq, np.zeros((B, 1), dtype=np.int32)], axis=1)).to(rep.device)
    seen[b, -1] = p
    logit = torch.ops.ader.score_items(rep[b:b + 1].contiguous(), table, torch.tensor([[p]], dtype=torch.int32, device=rep.device), N)
    logit = logit.cpu().numpy()[0, 0]
    out = {}
    for name, s in (("all", None), ("excluded", seen)):
        out[name] = [t.cpu().numpy() for t in torch.ops.ader.topk_items_stats(rep, table, s, N, k)]
    assert out["all"][0][b, 0] == p and p not in out["excluded"][0][b]
    assert out["excluded"][1][b, 0] < logit - 30.0
    for name in out:
        lse, ent = out[name][2], out[name][3]
        assert abs(float(lse[b]) - float(logit)) <= LSE_TOL_ULP * float(np.spacing(np.float32(abs(logit))))
        assert 0.0 <= ent[b] < 1e-6
    assert _same_bits(out["all"][2], out["excluded"][2]) and _same_bits(out["all"][3], out["excluded"][3])
    pr = np.exp(out["excluded"][1][b] - out["excluded"][2][b])
    assert pr.sum() < 1e-12                          # the probabilities of an answer need not sum to 1: here the mass is all excluded


# ---------------------------------------------------------------------------------------------- against trusted code
@pytest.mark.parametrize("i", [0, 1, 5])
def test_row_losses_are_lse_minus_the_target_score(i):
    eng, seq, lg, N, k, ref = _case(i)
    pos = np.random.RandomState(40 + i).randint(1, N + 1, size=seq.shape[0]).astype(np.int32)
    loss = eng.row_losses(seq, pos, N).cpu().numpy()
    lse = _fused(i, False)[2]
    mine = lse - eng.score_items(seq, pos[:, None], N)[:, 0]
    err = np.abs(loss.astype(np.float64) - mine.astype(np.float64)) / _ulp(ref[0])
    print("shape %d: worst |row_losses - (lse - score)| %.3f ulp at max(1, |lse|)" % (i, err.max()))
    assert err.max() <= LSE_TOL_ULP


# ---------------------------------------------------------------------------------------------- probabilities
def test_log_probs_and_probs():
    from ader_amd.engine.infer import log_probs, probs
    eng, seq, lg, N, k, ref = _case(2)                # N = 33, k = 64
    items, scores, lse, ent = _fused(2, False)
    lp, pr = log_probs(scores, lse), probs(scores, lse)
    assert _same_bits(lp, scores - lse[:, None])
    assert (items[:, N:] == 0).all() and np.isneginf(lp[:, N:]).all() and (pr[:, N:] == 0.0).all()      # padding: exactly 0
    assert (items[:, :N] > 0).all() and (pr[:, :N] > 0).all()
    it, sc, lse_n, _ = eng.recommend_stats(seq, N, N)  # k = N = 33: the whole distribution
    assert _same_bits(lse_n, lse) and np.array_equal(it, items[:, :N])
    total = probs(sc, lse_n).astype(np.float64).sum(axis=1)
    assert (np.abs(total - 1.0) <= N * 2.0 ** -24 + LSE_TOL_ULP * _ulp(ref[0])).all()
    it, sc, lse_x, _ = eng.recommend_stats(seq, N, N, exclude_seen=True)
    left = probs(sc, lse_x).astype(np.float64).sum(axis=1)
    assert (left < total - 1e-3).all()               # every session holds an item of 1..33: excluded items keep their mass


def _model(item_num, T, H=150):
    from ader_amd.model import Ader
    args = types.SimpleNamespace(maxlen=T, hidden_units=H, num_blocks=2, num_heads=1, random_seed=0, dropout_rate=0.3, l2_emb=0.0,
                                 disable_distillation=False, logits_dtype="f32")
    return Ader(item_num, args)


def test_ader_recommend_probs_routes():
    from ader_amd.engine.infer import log_probs, probs
    item_num, N, T = 400, 350, 50
    model = _model(item_num, T)
    eng = model.engine
    seq = _seqs(np.random.RandomState(2), 9, T, N)
    lse, ent = model.row_stats(seq, N)
    e_lse, e_ent = eng.row_stats(seq, N)
    assert _same_bits(lse, e_lse) and _same_bits(ent, e_ent)
    for exclude in (False, True):
        items, scores, f_lse, _ = eng.recommend_stats(seq, 20, N, exclude_seen=exclude)      # whole catalog, k <= 64: the fused call
        assert _same_bits(f_lse, lse)
        got = model.recommend_probs(seq, 20, N, exclude_seen=exclude)
        assert np.array_equal(got[0], items) and _same_bits(got[1], probs(scores, f_lse))
        got = model.recommend_probs(seq, 20, N, exclude_seen=exclude, form="logprob")
        assert np.array_equal(got[0], items) and _same_bits(got[1], log_probs(scores, f_lse))
        cand = np.arange(3, 300, 2)                                                             # candidates: recommend_among + row_stats
        items, scores = model.recommend(seq, 20, N, exclude_seen=exclude, dtype="f32", candidates=cand)
        got = model.recommend_probs(seq, 20, N, exclude_seen=exclude, candidates=cand)
        assert np.array_equal(got[0], items) and _same_bits(got[1], probs(scores, lse))
        items, scores = model.recommend(seq, 100, N, exclude_seen=exclude)                      # k > 64: recommend_wide + row_stats
        got = model.recommend_probs(seq, 100, N, exclude_seen=exclude, form="logprob")
        assert got[0].shape == (9, 100) and np.array_equal(got[0], items) and _same_bits(got[1], log_probs(scores, lse))
    for bad in ("probs", "logit", None):
        with pytest.raises(RuntimeError):
            model.recommend_probs(seq, 20, N, form=bad)
    with pytest.raises(RuntimeError):
        model.recommend_probs(seq, 0, N)
    eng.check_status()


# ---------------------------------------------------------------------------------------------- operators and the C ABI
@pytest.mark.parametrize("i", [0, 1, 3])
def test_operators_equal_the_engine_methods(i):
    import ader_amd.ops  # noqa: F401
    eng, seq, lg, N, k, ref = _case(i)
    rep = eng.encode(seq)
    emb = eng.param("emb").contiguous()
    lse, ent = (t.cpu().numpy() for t in torch.ops.ader.row_stats(rep, emb, N))
    assert _same_bits(lse, _fused(i, False)[2]) and _same_bits(ent, _fused(i, False)[3])
    seen = torch.from_numpy(np.array(seq)).to(rep.device)      # (a copy: the shared sessions are read-only)
    for exclude in (False, True):
        got = [t.cpu().numpy() for t in torch.ops.ader.topk_items_stats(rep, emb, seen if exclude else None, N, k)]
        for x, y in zip(got, _fused(i, exclude)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    with pytest.raises(RuntimeError):
        torch.ops.ader.topk_items_stats(rep, emb, None, N, 65)
    with pytest.raises(RuntimeError):
        torch.ops.ader.row_stats(rep, emb, emb.shape[0])


def test_errors():
    from ader_amd import _lib
    eng, seq, lg, N, k, ref = _case(2)
    for bad_k in (0, 65):
        with pytest.raises(RuntimeError):
            eng.recommend_stats(seq, bad_k, N)
    for bad_n in (0, eng.item_num + 1):
        with pytest.raises(RuntimeError):
            eng.recommend_stats(seq, 5, bad_n)
        with pytest.raises(RuntimeError):
            eng.row_stats(seq, bad_n)
    dev = eng.device
    rep = torch.zeros(64, eng.H, device=dev)
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    part = torch.zeros(_lib.call("ader_topk_ranges", N, 64) * 64 * 65, dtype=torch.int64, device=dev)
    spart = torch.zeros(_lib.call("ader_row_stats_floats", N, 64), device=dev)
    items, scores = torch.zeros(64, 65, dtype=torch.int32, device=dev), torch.zeros(64, 65, device=dev)
    lse, ent = torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for B, Bp, kk in ((64, 64, 65), (64, 64, 0), (64, 96, 5), (65, 64, 5)):
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_topk_items_stats", _lib.ptr(rep), eng._pp["emb"], B, Bp, eng.H, N, _lib.ptr(ncol), None, 0, kk, _lib.ptr(part),
                      _lib.ptr(spart), _lib.ptr(items), _lib.ptr(scores), _lib.ptr(lse), _lib.ptr(ent), st)
    for B, Bp in ((64, 96), (65, 64)):
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_row_stats", _lib.ptr(rep), eng._pp["emb"], B, Bp, eng.H, N, _lib.ptr(ncol), _lib.ptr(spart), _lib.ptr(lse),
                      _lib.ptr(ent), st)
    eng.check_status()
