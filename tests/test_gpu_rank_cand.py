"""Rank of a row's target among a candidate item list (Engine.rank_targets_among, Ader.rank_targets_among,
torch.ops.ader.rank_of_target_cand, ader_rank_targets_cand, Evaluator(candidates=..., exclude_seen=...)): the evaluation-side twin of
recommend_among.  The oracle is numpy on the device's own Engine.logits (oracle_ranks, checked on the host by
tests/test_rank_cand_host.py): non-candidate columns, seen columns under exclude_seen and the target's own column masked out, count of
(lg > tl) | ((lg == tl) & (id < t)).  No tolerance anywhere: ranks are compared with array_equal."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_rank_cand_host import oracle_ranks  # noqa: E402

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
SHAPES = [(700, 50, 150, 2, 1, 70, 650),              # rows over one chunk, N no multiple of 64
          (300, 20, 64, 1, 2, 9, 300),                # small batch, two heads
          (1000, 50, 150, 2, 3, 130, 777),            # three chunks
          (64, 8, 12, 1, 1, 3, 33),                   # less than one tile
          (2000, 20, 150, 1, 1, 1030, 1999),          # over MAX_ROWS: two engine chunks
          (40000, 20, 150, 1, 1, 70, 40000)]          # a workgroup walks several gathered tiles


@functools.lru_cache(maxsize=None)
def _case(i):
    """Engine, sessions, targets and the device logits of SHAPES[i]: computed once, shared, never written to."""
    item_num, T, H, L, heads, B, N = SHAPES[i]
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(6 + i)
    seq = _seqs(rs, B, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)           # random ids in [1, N]: some inside a list, some outside
    pos[1::5] = seq[1::5, -1]                                      # ... and some in the row's own seen ids
    lg = eng.logits(seq, N).cpu().numpy()
    for a in (lg, seq, pos):
        a.setflags(write=False)
    return eng, seq, pos, lg, N


def _patterns(i):
    """(name, list as handed to rank_targets_among, its ids within [1, N]) for SHAPES[i]."""
    item_num, N = SHAPES[i][0], SHAPES[i][6]
    rs = np.random.RandomState(40 + i)
    out = [("third", np.sort(rs.choice(N, size=max(N // 3, 1), replace=False)) + 1)]
    perm = rs.permutation(N) + 1
    for M in (0, 1, 63, 64, 65, 129):                  # an empty list, a single entry, both sides of a tile edge
        out.append(("first %d of a permutation" % M, np.sort(perm[:M])))
    out.append(("1..64 and every 97th", np.unique(np.concatenate([np.arange(1, min(64, N) + 1), np.arange(97, N + 1, 97)]))))
    above = np.arange(N + 1, item_num + 1)[::7]        # ids in (N, item_num]: legal, ignored (none where N == item_num)
    out.append(("ids above N", np.concatenate([out[0][1][::2], above])))
    if i == 5:
        out.append(("20000 spread", np.arange(1, N + 1, 2)))
    return [(name, c.astype(np.int64), c[c <= N]) for name, c in out]


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_all_ids_equal_rank_targets_and_the_oracle(i):
    eng, seq, pos, lg, N = _case(i)
    full = np.arange(1, N + 1)
    ref = oracle_ranks(lg, pos, full, None, False)
    whole = eng.rank_targets(seq, pos, N, dtype="f32")
    for got in (eng.rank_targets_among(seq, pos, N, full), eng.rank_targets_among(seq, pos, N)):
        assert got.dtype == np.int32 and got.shape == (seq.shape[0],)
        assert np.array_equal(got, whole) and np.array_equal(got, ref)
    # the whole catalog without the row's own items: the list is None
    assert np.array_equal(eng.rank_targets_among(seq, pos, N, exclude_seen=True), oracle_ranks(lg, pos, full, seq, True))
    eng.check_status()


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_candidate_patterns_equal_the_masked_count(i, exclude):
    from ader_amd._lib import call
    eng, seq, pos, lg, N = _case(i)
    Bp = (min(seq.shape[0], eng.MAX_ROWS) + 63) // 64 * 64
    for name, given, inside in _patterns(i):
        got = eng.rank_targets_among(seq, pos, N, given, exclude_seen=exclude)
        assert got.dtype == np.int32 and np.array_equal(got, oracle_ranks(lg, pos, inside, seq, exclude)), name
        assert (got <= len(inside)).all(), name
        if len(inside) == 0:
            assert not got.any(), name
        if name == "20000 spread":                     # a workgroup walks several gathered tiles: its counts carry over
            assert len(inside) == 20000 and (len(inside) + 63) // 64 > call("ader_topk_ranges", len(inside), Bp)
    eng.check_status()


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("i", [0, 2, 3])
def test_round_trip_with_recommend_among(i, exclude):
    """rank_targets_among(seq_b, items[b, j]) == j for what recommend_among returns over the same list: all n * k pairs in one call."""
    eng, seq, pos, lg, N = _case(i)
    k = 20
    cand = _patterns(i)[0][1]
    items, _ = eng.recommend_among(seq, k, cand, N, exclude_seen=exclude)
    n = seq.shape[0]
    rows = np.repeat(np.arange(n), k)
    tg = items.reshape(-1)
    live = tg > 0
    assert live[::k].all()                             # every row has a best item
    got = eng.rank_targets_among(np.ascontiguousarray(seq[rows][live]), np.ascontiguousarray(tg[live]), N, cand, exclude_seen=exclude)
    assert np.array_equal(got, np.tile(np.arange(k), n)[live])


def test_planted_ties_count_the_lower_ids_only_and_a_tied_item_left_out_not_at_all():
    item_num, T, H, L, heads, B, N = SHAPES[0]
    eng = _engine(item_num, T, H, L, heads)
    seq = _case(0)[1]
    t = 411                                            # row 0's target, tied with four items spread over the catalog's tiles
    emb = eng.param("emb")
    tied = sorted([t, 3, 200, N - 2, 500])
    for j in tied:
        emb[j] = emb[t]
    eng.refresh_shadow()
    left_out = 200
    rs = np.random.RandomState(9)
    cand = np.unique(np.concatenate([rs.choice(N, size=150, replace=False) + 1, tied]))
    cand = cand[cand != left_out]
    lg = eng.logits(seq, N).cpu().numpy()
    assert len(set(lg[0, np.array(tied) - 1].view(np.int32).tolist())) == 1
    pos = _case(0)[2].copy()
    pos[0] = t
    for exclude in (False, True):
        got = eng.rank_targets_among(seq, pos, N, cand, exclude_seen=exclude)
        assert np.array_equal(got, oracle_ranks(lg, pos, cand, seq, exclude))
    above = int(np.count_nonzero(lg[0, cand - 1] > lg[0, t - 1]))
    got = eng.rank_targets_among(seq, pos, N, cand)
    assert got[0] == above + 1                         # item 3 (tied, lower id, listed); not 200 (left out), not 500 and N - 2 (higher ids)
    with_it = eng.rank_targets_among(seq, pos, N, np.append(cand, left_out))
    assert with_it[0] == above + 2                     # listed, it counts: the tie was real
    # a target that is in its own seen list still ranks under exclude_seen
    seq2 = seq.copy()
    seq2[0, -1] = t
    lg2 = eng.logits(seq2, N).cpu().numpy()
    got2 = eng.rank_targets_among(seq2, pos, N, cand, exclude_seen=True)
    assert np.array_equal(got2, oracle_ranks(lg2, pos, cand, seq2, True))
    tl = lg2[0, t - 1]
    seen0 = seq2[0][seq2[0] > 0]
    c0 = cand[~np.isin(cand, seen0)]
    assert got2[0] == np.count_nonzero((lg2[0, c0 - 1] > tl) | ((lg2[0, c0 - 1] == tl) & (c0 < t)))


def _op(rep, emb, target, cand, seen, N):
    import ader_amd.ops  # noqa: F401
    dev = torch.device("cuda")
    as_dev = lambda x, dt: x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=dt)).to(dev)
    s = None if seen is None else as_dev(seen, np.int32)
    rk = torch.ops.ader.rank_of_target_cand(as_dev(rep, np.float32), as_dev(emb, np.float32), as_dev(target, np.int32),
                                            as_dev(cand, np.int32), s, N)
    assert rk.dtype == torch.int32 and rk.shape == (len(target),)
    return rk.cpu().numpy()


def test_raw_op_raises_on_a_list_that_is_not_strictly_ascending():
    eng, seq, pos, lg, N = _case(0)
    rep, emb = eng.encode(seq), eng.param("emb")
    good = np.arange(5, 400, 3)                        # every id inside [1, N]: even a faulty kernel reads only inside the table
    for bad in (good[::-1].copy(), np.concatenate([good[:70], good[69:]]), np.concatenate([good[:100], good[:30]])):
        assert bad.min() >= 1 and bad.max() <= N
        with pytest.raises(RuntimeError, match="ascending"):
            _op(rep, emb, pos, bad, None, N)
    assert np.array_equal(_op(rep, emb, pos, good, None, N), oracle_ranks(lg, pos, good, seq, False))


@pytest.mark.parametrize("with_seen", [False, True])
def test_raw_op_ignores_ids_above_n(with_seen):
    eng, seq, pos, lg, N = _case(0)                    # N = 650 of item_num = 700
    rep, emb = eng.encode(seq), eng.param("emb")
    cand = np.arange(2, eng.item_num + 1, 3)
    assert (cand > N).any() and cand.max() <= eng.item_num
    got = _op(rep, emb, pos, cand, seq if with_seen else None, N)
    assert np.array_equal(got, oracle_ranks(lg, pos, cand[cand <= N], seq, with_seen))


def test_total_tie_ranks_by_the_number_of_lower_candidate_ids():
    rs = np.random.RandomState(2)
    B, N, H = 70, 650, 150
    emb = (rs.standard_normal((N + 1, H)) * 0.05).astype(np.float32)
    rep = rs.standard_normal((B, H)).astype(np.float32)
    rep[::2] = 0.0                                     # all-zero rep rows: every score is +0
    cand = np.sort(rs.choice(N, size=300, replace=False)) + 1
    target = rs.randint(1, N + 1, size=B).astype(np.int32)
    target[0], target[2] = cand[17], cand[0]
    got = _op(rep, emb, target, cand, None, N)
    assert got[::2].tolist() == [int(np.count_nonzero(cand < t)) for t in target[::2]]
    lg = (rep.astype(np.float64) @ emb[1:].T.astype(np.float64)).astype(np.float32)
    assert np.array_equal(got[::2], oracle_ranks(lg[::2], target[::2], cand, None, False))


def test_an_unsorted_list_with_duplicates_is_the_normalised_list():
    from ader_amd.engine.infer import candidate_ids
    eng, seq, pos, lg, N = _case(0)
    rs = np.random.RandomState(12)
    raw = rs.randint(1, eng.item_num + 1, size=400)
    raw = np.concatenate([raw, raw[:50]])
    assert len(np.unique(raw)) < len(raw) and (np.diff(raw) < 0).any() and (raw > N).any()
    norm = candidate_ids(raw, N, eng.item_num)
    a = eng.rank_targets_among(seq, pos, N, raw)
    for other in (norm, torch.from_numpy(raw), raw.tolist(), torch.from_numpy(raw.astype(np.int32)).to(eng.device)):
        assert eng.rank_targets_among(seq, pos, N, other).tobytes() == a.tobytes()
    assert np.array_equal(a, oracle_ranks(lg, pos, norm, seq, False))


@pytest.mark.parametrize("exclude", [False, True])
def test_calls_repeat_and_rows_are_independent(exclude):
    eng, seq, pos, lg, N = _case(2)
    cand = _patterns(2)[0][1]
    a = eng.rank_targets_among(seq, pos, N, cand, exclude_seen=exclude)
    b = eng.rank_targets_among(seq, pos, N, cand, exclude_seen=exclude)
    assert a.tobytes() == b.tobytes()
    perm = np.random.RandomState(3).permutation(seq.shape[0])
    c = eng.rank_targets_among(np.ascontiguousarray(seq[perm]), np.ascontiguousarray(pos[perm]), N, cand, exclude_seen=exclude)
    assert np.array_equal(c, a[perm])


def test_engine_and_model_surface():
    from ader_amd.main import build_parser
    from ader_amd.model import Ader
    eng, seq, pos, lg, N = _case(3)
    for bad in ([0, 3], [-1, 3], [3, eng.item_num + 1], np.array([1.0, 2.0]), np.array([[1, 2]])):
        with pytest.raises(RuntimeError):
            eng.rank_targets_among(seq, pos, N, bad)
    for bad_n in (0, eng.item_num + 1):
        with pytest.raises(RuntimeError, match="max_item"):
            eng.rank_targets_among(seq, pos, bad_n, [1, 2])
    eng.check_status()
    args = build_parser().parse_args(["--hidden_units", "12", "--maxlen", "8", "--num_blocks", "1"])
    model = Ader(64, args)
    cand = [9, 2, 30, 2]
    got = model.rank_targets_among(seq, pos, N, cand, True)
    assert np.array_equal(got, model.engine.rank_targets_among(seq, pos, N, candidates=cand, exclude_seen=True))
    assert np.array_equal(model.rank_targets_among(seq, pos, N), model.rank_targets(seq, pos, N))


def test_launcher_errors_return_minus_two_and_leave_the_status_alone():
    from ader_amd import _lib
    eng, seq, pos, lg, N = _case(3)
    dev = eng.device
    cand = np.arange(1, N + 1, 2)
    M = len(cand)
    cand_d = torch.from_numpy(cand.astype(np.int32)).to(dev)
    rep = torch.zeros(64, eng.H, device=dev)
    ncol = torch.full((64,), N, dtype=torch.int32, device=dev)
    tgt = torch.ones(64, dtype=torch.int32, device=dev)
    tl, rk = torch.zeros(64, device=dev), torch.full((64,), 7, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    for c, m in ((_lib.ptr(cand_d), -1), (None, M)):
        with pytest.raises(_lib.AderHipError, match="code -2"):
            _lib.call("ader_rank_targets_cand", _lib.ptr(rep), eng._pp["emb"], 64, 64, eng.H, N, _lib.ptr(tgt), _lib.ptr(ncol), c, m,
                      None, 0, _lib.ptr(tl), _lib.ptr(rk), _lib.ptr(status), st)
    assert int(status.item()) == 0 and (rk == 7).all()             # nothing was enqueued
    _lib.call("ader_rank_targets_cand", _lib.ptr(rep), eng._pp["emb"], 64, 64, eng.H, N, _lib.ptr(tgt), _lib.ptr(ncol), None, 0,
              None, 0, _lib.ptr(tl), _lib.ptr(rk), _lib.ptr(status), st)
    assert int(status.item()) == 0 and not rk.any()                # M = 0: the clear of rank


def test_driver_eval_among_period_adds_a_line_and_summary_keys():
    """One period, one epoch of the finetune baseline with --eval_among period: the test line is followed by the line among the
    period's own items, and the summary entry gains the among_* keys beside the untouched ones.  A listed subset can only take
    items away from ahead of a target, so every rank among the list is <= the catalog rank: the metrics cannot fall."""
    import tempfile

    from ader_amd import main as M
    from ader_amd.data import DataLoader
    with tempfile.TemporaryDirectory() as d:
        args = M.build_parser().parse_args(["--dataset", "DIGINETICA", "--max_periods", "1", "--num_epochs", "1", "--finetune", "True",
                                            "--eval_among", "period", "--results_root", d])
        out = M.run(args, log=lambda s="": None)
        text = open(os.path.join(d, "DIGINETICA-ADER", "Training_logs.txt")).read().splitlines()
    (p,) = out["periods"]
    dl = DataLoader("DIGINETICA")
    train, _ = dl.train_loader(0)
    assert p["among_items"] == len(M.period_items(train, dl.max_item())) and 0 < p["among_items"] <= p["max_item"]
    i = [n for n, l in enumerate(text) if l.startswith("epoch:1, test (MRR@20: ")]
    assert len(i) == 1 and text[i[0] + 1].startswith("epoch:1, test among %d candidate items (MRR@20: " % p["among_items"])
    assert text[i[0] + 1].endswith("(MRR@20: %.4f, RECALL@20: %.4f, MRR@10: %.4f, RECALL@10: %.4f)"
                                   % (p["among_mrr20"], p["among_recall20"], p["among_mrr10"], p["among_recall10"]))
    assert set(p) == {"period", "best_epoch", "mrr20", "recall20", "mrr10", "recall10", "max_item",
                      "among_mrr20", "among_recall20", "among_mrr10", "among_recall10", "among_items"}
    for k in ("mrr20", "recall20", "mrr10", "recall10"):
        assert 0.0 < p[k] <= p["among_" + k] <= 1.0
    assert out["average"]["recall20"] == p["recall20"]


def test_evaluator_fills_ranks_among_and_leaves_its_default_output_alone(capsys):
    import random

    from ader_amd.data import Evaluator, recall_mrr
    from ader_amd.main import build_parser
    from ader_amd.model import Ader
    item_num, T, H, L, heads, B, N = SHAPES[0]
    rs = np.random.RandomState(4)
    sessions = [[int(x) for x in rs.randint(1, N + 1, size=int(rs.randint(2, 12)))] for _ in range(60)]
    cand = np.unique(rs.randint(1, N + 1, size=250))
    args = build_parser().parse_args(["--hidden_units", str(H), "--maxlen", str(T), "--num_blocks", str(L), "--num_heads", str(heads)])
    model = Ader(item_num, args)
    random.seed(9)
    plain = Evaluator(sessions, False, T, 64, N, "test", model, None)
    plain_info = plain.evaluate(2)
    plain_out = capsys.readouterr().out
    for exclude in (False, True):
        random.seed(9)
        ev = Evaluator(sessions, False, T, 64, N, "test", model, None, candidates=cand, exclude_seen=exclude)
        info = ev.evaluate(2)
        assert capsys.readouterr().out == plain_out and info == plain_info
        assert ev.ranks == plain.ranks and ev.results() == plain.results()
        # the rows of the pass, again: the same seed gives the same batches
        random.seed(9)
        smp = Evaluator(sessions, False, T, 64, N, "test", model, None).evaluate_sampler
        batches = [smp.next_batch() for _ in range(smp.batch_num())]
        seq = np.concatenate([s for s, p in batches if len(p)])
        pos = np.concatenate([p for s, p in batches if len(p)])
        assert len(pos) == len(ev.ranks_among) > 60
        assert ev.ranks_among == model.engine.rank_targets_among(seq, pos, N, cand, exclude_seen=exclude).tolist()
        ref = oracle_ranks(model.engine.logits(seq, N).cpu().numpy(), pos, cand, seq, exclude)
        assert ev.ranks_among == ref.tolist() and ev.results_among() == recall_mrr(ref)
        line = ev.display_among(2)
        assert "among %d candidate items" % len(cand) in line and capsys.readouterr().out == line + "\n"
