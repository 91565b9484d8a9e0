"""Host side of the per-row item lists (no GPU): row_candidate_ids, the rank contract stated in numpy against the stable argsort of a masked
score matrix, sample_negatives, the signatures of the new methods, the --eval_negatives flag, the Evaluator's sampled pass over a stub
model, and the ctypes table of the four new symbols."""
import inspect
import os
import random

import numpy as np
import pytest
import torch


def oracle_ranks_rows(lg, pos, lists, seen, exclude):
    """The contract of rank_targets_per_row in numpy: lg [n,N] scores, pos [n] targets, lists = per row the ids within [1, N], seen [n,S]
    ids (0 = none, ids above N ignored) -> int32 [n]: listed, unseen ids other than the target that precede it by (score descending, id
    ascending)."""
    lg = np.asarray(lg, dtype=np.float32)
    n, N = lg.shape
    ids = np.arange(1, N + 1)
    out = np.zeros(n, dtype=np.int32)
    for b in range(n):
        m = np.zeros(N, dtype=bool)
        c = np.asarray(lists[b], dtype=np.int64)
        m[c[(c >= 1) & (c <= N)] - 1] = True
        if exclude:
            s = np.asarray(seen[b])
            m[s[(s > 0) & (s <= N)] - 1] = False
        t = int(pos[b])
        m[t - 1] = False
        tl = lg[b, t - 1]
        out[b] = np.count_nonzero(m & ((lg[b] > tl) | ((lg[b] == tl) & (ids < t))))
    return out


# ------------------------------------------------------------------------------------------------ row_candidate_ids
def test_row_candidate_ids_ragged_2d_and_tensors():
    from ader_amd.engine.infer import row_candidate_ids
    got = row_candidate_ids([[5, 3, 3, 900], [], [1, 2], [7]], 100, 1000)
    assert got.dtype == np.int32 and got.tolist() == [[3, 5], [0, 0], [1, 2], [7, 0]]
    two_d = np.array([[9, 0, 4, 4], [0, 0, 0, 0], [1, 2, 3, 4]], dtype=np.int64)
    ref = [[4, 9, 0, 0], [0, 0, 0, 0], [1, 2, 3, 4]]
    for form in (two_d, torch.from_numpy(two_d), torch.from_numpy(two_d.astype(np.int32)), two_d.tolist(),
                 [torch.tensor(r) for r in two_d.tolist()], [np.array(r, dtype=np.int16) for r in two_d.tolist()]):
        got = row_candidate_ids(form, 100, 1000)
        assert got.dtype == np.int32 and got.tolist() == ref
    assert row_candidate_ids([[], []], 5, 9).shape == (2, 0)
    assert row_candidate_ids(np.zeros((3, 4), dtype=np.int32), 5, 9).shape == (3, 0)
    assert row_candidate_ids([], 5, 9).shape == (0, 0)


def test_row_candidate_ids_drops_ids_above_n_and_is_the_identity_on_its_own_form():
    from ader_amd.engine.infer import row_candidate_ids
    got = row_candidate_ids([[2, 50, 51, 99], [60, 70]], 50, 100)
    assert got.tolist() == [[2, 50], [0, 0]]
    rs = np.random.RandomState(0)
    raw = rs.randint(0, 301, size=(40, 30))
    norm = row_candidate_ids(raw, 250, 300)
    assert np.array_equal(row_candidate_ids(norm, 250, 300), norm)
    for b in range(40):
        want = np.unique(raw[b][(raw[b] > 0) & (raw[b] <= 250)])
        assert norm[b, :len(want)].tolist() == want.tolist() and not norm[b, len(want):].any()
    # a row already in form is not sorted again: np.unique is never reached
    import ader_amd.engine.infer as I
    real = np.unique
    try:
        np.unique = None
        assert np.array_equal(I.row_candidate_ids(norm, 250, 300), norm)
        assert I.row_candidate_ids([[1, 4, 9], [2]], 250, 300).tolist() == [[1, 4, 9], [2, 0, 0]]
    finally:
        np.unique = real


def test_row_candidate_ids_errors():
    from ader_amd.engine.infer import row_candidate_ids
    for bad in (np.array([[1.0, 2.0]]), np.array([1, 2, 3]), np.zeros((2, 2, 2), dtype=np.int32), [[1, -1]], [[1, 11]], [[1.5]],
                [[[1, 2]]], torch.tensor([[0.5]])):
        with pytest.raises(RuntimeError):
            row_candidate_ids(bad, 5, 10)


# ------------------------------------------------------------------------------------------------ the rank contract
def test_rank_oracle_is_the_position_in_the_masked_stable_argsort():
    rs = np.random.RandomState(3)
    n, N, S = 40, 90, 6
    lg = rs.randint(-4, 5, size=(n, N)).astype(np.float32)         # few distinct values: many ties
    seen = rs.randint(0, N + 1, size=(n, S))
    lists = [np.unique(rs.randint(1, N + 1, size=int(rs.randint(0, 60)))) for _ in range(n)]
    pos = rs.randint(1, N + 1, size=n)
    pos[::3] = [l[0] if len(l) else 1 for l in lists[::3]]         # listed targets, unlisted ones, and (below) seen ones
    pos[1::7] = np.maximum(seen[1::7, 0], 1)
    for exclude in (False, True):
        got = oracle_ranks_rows(lg, pos, lists, seen, exclude)
        for b in range(n):
            m = np.full(N, -np.inf, dtype=np.float32)
            keep = set(lists[b].tolist())
            if exclude:
                keep -= set(seen[b].tolist())
            keep.add(int(pos[b]))                                  # the target is ranked among the others, whatever it is itself
            idx = np.array(sorted(keep)) - 1
            m[idx] = lg[b, idx]
            order = np.argsort(-m, kind="stable")
            assert got[b] == int(np.nonzero(order == pos[b] - 1)[0][0]), (b, exclude)


# ------------------------------------------------------------------------------------------------ sample_negatives
def test_sample_negatives_rows_are_distinct_ascending_unseen_and_deterministic():
    from ader_amd.data import sample_negatives
    rs = np.random.RandomState(5)
    n, T, n_neg = 300, 12, 100
    max_item = n_neg + T + 1 + 7
    seq = rs.randint(0, max_item + 1, size=(n, T)).astype(np.int32)
    pos = rs.randint(1, max_item + 1, size=n).astype(np.int32)
    py, npst = random.getstate(), np.random.get_state()
    a = sample_negatives(seq, pos, max_item, n_neg, 7)
    assert random.getstate() == py
    now = np.random.get_state()
    assert now[0] == npst[0] and np.array_equal(now[1], npst[1]) and now[2:] == npst[2:]
    assert a.dtype == np.int32 and a.shape == (n, n_neg)
    assert (np.diff(a, axis=1) > 0).all() and a.min() >= 1 and a.max() <= max_item
    for b in range(n):
        assert pos[b] not in a[b] and not np.isin(a[b], seq[b][seq[b] > 0]).any()
    assert np.array_equal(a, sample_negatives(torch.from_numpy(seq), torch.from_numpy(pos), max_item, n_neg, 7))
    assert not np.array_equal(a, sample_negatives(seq, pos, max_item, n_neg, 8))
    # exactly n_neg eligible ids: the row is all of them
    one = sample_negatives(np.array([[0, 2, 2]]), [4], 6, 4, 0)
    assert one.tolist() == [[1, 3, 5, 6]]


def test_sample_negatives_is_uniform_over_the_eligible_ids():
    from ader_amd.data import sample_negatives
    seq = np.tile(np.array([[0, 3, 7]]), (20000, 1))
    got = sample_negatives(seq, np.full(20000, 5), 12, 3, 1)
    cnt = np.bincount(got.ravel(), minlength=13)
    assert cnt[[0, 3, 5, 7]].sum() == 0
    el = cnt[[1, 2, 4, 6, 8, 9, 10, 11, 12]]
    # 60,000 draws over 9 ids: mean 6,667, standard deviation below 77 (binomial, p = 1/3 per row): six of them
    assert np.abs(el - 60000 / 9).max() < 6 * 77


def test_sample_negatives_raises_when_a_row_is_short():
    from ader_amd.data import sample_negatives
    with pytest.raises(RuntimeError, match="fewer than"):
        sample_negatives(np.array([[1, 2, 3]]), [4], 8, 5, 0)
    with pytest.raises(RuntimeError):
        sample_negatives(np.array([1, 2, 3]), [4], 80, 5, 0)


# ------------------------------------------------------------------------------------------------ surface
def test_signatures_of_the_new_methods():
    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    sig = lambda f: str(inspect.signature(f))
    assert sig(Engine.score_items) == "(self, seq, items, max_item=None)"
    assert sig(Engine.recommend_per_row) == "(self, seq, k, lists, max_item=None, exclude_seen=False)"
    assert sig(Engine.rank_targets_per_row) == "(self, seq, pos, max_item, lists, exclude_seen=False)"
    assert sig(Ader.score_items) == sig(Engine.score_items)
    assert sig(Ader.recommend_per_row) == sig(Engine.recommend_per_row)
    assert sig(Ader.rank_targets_per_row) == sig(Engine.rank_targets_per_row)


def test_eval_negatives_flag():
    from ader_amd.main import _BUILD_FLAGS, build_parser
    flag = [f for f in _BUILD_FLAGS if f[0] == "eval_negatives"]
    assert len(flag) == 1 and flag[0][1] == 0 and flag[0][2] is int
    assert build_parser().parse_args([]).eval_negatives == 0
    assert build_parser().parse_args(["--eval_negatives", "100"]).eval_negatives == 100
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--eval_negatives", "many"])


class _Stub:
    """A model of the Evaluator's fast paths: ranks are a function of the row, calls are recorded."""

    def __init__(self):
        self.calls = []

    def rank_targets(self, seq, pos, max_item):
        return (np.asarray(pos) % 7).astype(np.int32)

    def rank_targets_per_row(self, seq, pos, max_item, lists, exclude_seen=False):
        self.calls.append((np.array(seq), np.array(pos), max_item, np.array(lists), exclude_seen))
        return (np.asarray(pos) % 3).astype(np.int32)


def test_evaluator_sampled_pass_over_a_stub_model(capsys):
    from ader_amd.data import Evaluator, recall_mrr, sample_negatives
    rs = np.random.RandomState(4)
    T, N = 10, 200
    sessions = [[int(x) for x in rs.randint(1, N + 1, size=int(rs.randint(2, 9)))] for _ in range(150)]
    random.seed(9)
    plain = Evaluator(sessions, False, T, 64, N, "test", _Stub(), None)
    plain_info = plain.evaluate(3)
    plain_out = capsys.readouterr().out
    with pytest.raises(RuntimeError):
        plain.results_sampled()
    stub = _Stub()
    random.seed(9)
    ev = Evaluator(sessions, False, T, 64, N, "test", stub, None, negatives=50, neg_seed=3)
    info = ev.evaluate(3)
    assert info == plain_info and capsys.readouterr().out == plain_out
    assert ev.ranks == plain.ranks and ev.results() == plain.results()
    assert len(stub.calls) == 1                                    # the concatenated rows, once
    seq, pos, max_item, lists, exclude = stub.calls[0]
    random.seed(9)
    smp = Evaluator(sessions, False, T, 64, N, "test", _Stub(), None).evaluate_sampler
    batches = [smp.next_batch() for _ in range(smp.batch_num())]
    assert np.array_equal(seq, np.concatenate([s for s, p in batches if len(p)]))
    assert np.array_equal(pos, np.concatenate([p for s, p in batches if len(p)]))
    assert len(pos) == len(ev.ranks) > 64 and max_item == N and exclude is False
    assert np.array_equal(lists, sample_negatives(seq, pos, N, 50, 3)) and lists.shape == (len(pos), 50)
    assert ev.ranks_sampled == (pos % 3).tolist()
    assert ev.results_sampled() == recall_mrr(ev.ranks_sampled)
    line = ev.display_sampled(3)
    assert capsys.readouterr().out == line + "\n"
    assert line == ("epoch:3, test among the target and 50 sampled unseen items (MRR@20: %.4f, RECALL@20: %.4f, MRR@10: %.4f, "
                    "RECALL@10: %.4f)" % ev.results_sampled())


def test_evaluator_with_negatives_needs_rank_targets_per_row():
    from ader_amd.data import Evaluator

    class Old:
        def rank_targets(self, seq, pos, max_item):
            return np.zeros(len(pos), dtype=np.int32)

    sessions = [[1, 2, 3], [4, 5]]
    Evaluator(sessions, False, 5, 8, 10, "test", Old(), None)
    with pytest.raises(RuntimeError, match="rank_targets_per_row"):
        Evaluator(sessions, False, 5, 8, 10, "test", Old(), None, negatives=3)


def test_ctypes_argument_counts_of_the_new_symbols():
    from ader_amd import _lib
    want = {"ader_score_items": 12, "ader_topk_items_rows": 18, "ader_rank_targets_rows": 17, "ader_topk_rows_ranges": 2}
    for name, n in want.items():
        assert len(_lib._SIGS[name]) == n, name
    assert "ader_topk_rows_ranges" in _lib._NO_CHECK
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ader_hip.h")).read()
    for name in want:
        assert "int %s(" % name in hdr


def test_the_three_operators_trace_under_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode

    from ader_amd import build
    build.build()
    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        rep, emb, ids = torch.empty(5, 150), torch.empty(101, 150), torch.empty(5, 40, dtype=torch.int32)
        seen, tgt = torch.empty(5, 50, dtype=torch.int32), torch.empty(5, dtype=torch.int32)
        s = torch.ops.ader.score_items(rep, emb, ids, 100)
        assert tuple(s.shape) == (5, 40) and s.dtype == torch.float32
        for sn in (None, seen):
            items, scores = torch.ops.ader.topk_items_rows(rep, emb, ids, sn, 100, 33)
            assert tuple(items.shape) == (5, 33) and items.dtype == torch.int32
            assert tuple(scores.shape) == (5, 33) and scores.dtype == torch.float32
            rk = torch.ops.ader.rank_of_target_rows(rep, emb, tgt, ids, sn, 100)
            assert tuple(rk.shape) == (5,) and rk.dtype == torch.int32
    doc = ader_amd.ops.__doc__
    for name in ("ader::score_items(", "ader::topk_items_rows(", "ader::rank_of_target_rows("):
        assert name in doc


def test_rows_ranges_is_the_ceiling_and_at_least_one():
    from ader_amd import build
    import ctypes
    build.build()
    import torch  # noqa: F401, F811  (one HIP runtime for the process, see ader_amd/_lib.py)
    lib = ctypes.CDLL(build.LIB)
    for C, k, want in ((0, 20, 1), (1, 20, 1), (20, 20, 1), (21, 20, 2), (1024, 64, 16), (65, 64, 2), (300, 1, 300)):
        assert lib.ader_topk_rows_ranges(C, k) == want
