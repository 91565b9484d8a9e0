"""Host side of the candidate-list rank (Engine.rank_targets_among, ader_rank_targets_cand): the numpy oracle that
tests/test_gpu_rank_cand.py holds the kernel to, checked here against an independent statement of the same contract; the signatures,
the driver flag and the export; the Evaluator's new arguments with a stub model.  No GPU."""
import inspect
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_ranks(lg, target, cand, seen, exclude):
    """The contract of ader_rank_targets_cand in numpy.  lg [n,N] float32 scores of items 1..N, target [n] ids in [1, N], cand: ids in
    [1, N] (any order, duplicates allowed), seen [n,S] ids (0 = none, ids above N ignored) or None -> int32 [n]: the number of listed
    items, other than the target and -- under exclude -- the row's seen ids, with lg > the target's, or == and a lower id."""
    lg = np.asarray(lg, dtype=np.float32)
    n, N = lg.shape
    ids = np.arange(1, N + 1)
    listed = np.zeros(N, dtype=bool)
    listed[np.asarray(cand, dtype=np.int64) - 1] = True
    out = np.zeros(n, dtype=np.int32)
    for b in range(n):
        m = listed.copy()
        if exclude:
            s = np.asarray(seen[b])
            m[s[(s > 0) & (s <= N)] - 1] = False
        t = int(target[b])
        m[t - 1] = False
        tl = lg[b, t - 1]
        out[b] = np.count_nonzero(m & ((lg[b] > tl) | ((lg[b] == tl) & (ids < t))))
    return out


def _argsort_rank(row, t, cand, seen_row, exclude):
    """The independent statement: every column that is not a candidate of the row goes to -inf, the target's own column keeps its
    score, and the rank is the target's index in the stable argsort of the negated row."""
    N = len(row)
    r = np.full(N, -np.inf, dtype=np.float32)
    keep = np.unique(np.asarray(cand, dtype=np.int64))
    if exclude:
        keep = np.setdiff1d(keep, seen_row[(seen_row > 0) & (seen_row <= N)])
    r[keep - 1] = row[keep - 1]
    r[t - 1] = row[t - 1]
    order = np.argsort(-r, kind="stable")
    return int(np.nonzero(order == t - 1)[0][0])


@pytest.mark.parametrize("exclude", [False, True])
def test_oracle_is_the_target_index_in_the_stable_argsort_of_the_masked_row(exclude):
    rs = np.random.RandomState(5)
    n, N, S = 60, 97, 9
    lg = (rs.randint(-4, 5, size=(n, N)) / 4.0).astype(np.float32)       # nine distinct values: every row is full of equal entries
    assert all(len(np.unique(lg[b])) < N for b in range(n))
    seen = rs.randint(0, N + 6, size=(n, S)).astype(np.int32)            # zeros and ids above N among them
    cand = np.sort(rs.choice(N, size=40, replace=False)) + 1
    target = rs.randint(1, N + 1, size=n).astype(np.int32)
    target[:10] = cand[rs.randint(0, len(cand), size=10)]                # inside the list
    outside = np.setdiff1d(np.arange(1, N + 1), cand)
    target[10:20] = outside[rs.randint(0, len(outside), size=10)]        # outside it
    for b in range(20, 30):                                              # in the row's own seen list, listed (b even) or not
        target[b] = cand[b] if b % 2 == 0 else outside[b]
        seen[b, b % S] = target[b]
    for c in (cand, cand[::-1].tolist() + cand[:5].tolist(), np.arange(1, N + 1), cand[:1], np.zeros(0, dtype=np.int64)):
        got = oracle_ranks(lg, target, c, seen, exclude)
        assert got.dtype == np.int32 and got.shape == (n,)
        want = [_argsort_rank(lg[b], int(target[b]), c, seen[b], exclude) for b in range(n)]
        assert got.tolist() == want
        if len(c) == 0:
            assert not got.any()
    # with every item listed and nothing excluded it is the whole-catalog rank: the index in the plain stable argsort
    full = oracle_ranks(lg, target, np.arange(1, N + 1), None, False)
    plain = [int(np.nonzero(np.argsort(-lg[b], kind="stable") == target[b] - 1)[0][0]) for b in range(n)]
    assert full.tolist() == plain


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_signatures():
    from ader_amd.engine import Engine
    from ader_amd.model import Ader
    E = inspect.Parameter.empty
    want = [("self", E), ("seq", E), ("pos", E), ("max_item", E), ("candidates", None), ("exclude_seen", False)]
    assert _params(Engine.rank_targets_among) == want
    assert _params(Ader.rank_targets_among) == want
    # what exists stays as it is
    assert _params(Engine.rank_targets) == [("self", E), ("seq", E), ("pos", E), ("max_item", E), ("dtype", None), ("cand_cap", None)]
    assert _params(Ader.rank_targets) == [("self", E), ("seq", E), ("pos", E), ("max_item", E)]
    assert _params(Engine.recommend) == [("self", E), ("seq", E), ("k", E), ("max_item", None), ("exclude_seen", False), ("dtype", None),
                                         ("band", None)]
    assert _params(Engine.recommend_among) == [("self", E), ("seq", E), ("k", E), ("candidates", E), ("max_item", None),
                                               ("exclude_seen", False), ("dtype", None)]
    assert _params(Engine.recommend_wide) == [("self", E), ("seq", E), ("k", E), ("max_item", None), ("exclude_seen", False), ("cap", None)]
    assert _params(Ader.recommend) == [("self", E), ("seq", E), ("k", E), ("max_item", None), ("exclude_seen", False), ("dtype", None),
                                       ("candidates", None)]


def test_eval_among_flag():
    from ader_amd.main import _BUILD_FLAGS, build_parser
    flag = [f for f in _BUILD_FLAGS if f[0] == "eval_among"]
    assert len(flag) == 1 and flag[0][1] == "catalog" and flag[0][2] is str and flag[0][3] == ("catalog", "period")
    assert build_parser().parse_args([]).eval_among == "catalog"
    assert build_parser().parse_args(["--eval_among", "period"]).eval_among == "period"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--eval_among", "category"])


def test_period_items_are_the_distinct_ids_up_to_max_item():
    from ader_amd.data import PackedSessions
    from ader_amd.main import period_items
    sessions = [[5, 3, 9], [3, 12, 5], [40, 1]]
    for s in (sessions, PackedSessions.from_lists(sessions)):
        got = period_items(s, 12)
        assert got.tolist() == [1, 3, 5, 9, 12] and np.issubdtype(got.dtype, np.integer)
    assert period_items([], 12).tolist() == []


def test_export_is_declared_bound_and_built():
    from ader_amd import _lib
    header = open(os.path.join(ROOT, "include", "ader_hip.h")).read()
    assert "int ader_rank_targets_cand(" in header
    assert "ader_rank_targets_cand" in _lib.exported_symbols()
    assert len(_lib._SIGS["ader_rank_targets_cand"]) == 16               # the C declaration's parameters
    if os.path.isfile(_lib.LIB_PATH):
        import ctypes
        assert ctypes.CDLL(_lib.LIB_PATH).ader_rank_targets_cand is not None      # (AttributeError: the symbol is missing)


class _Stub:
    """Records its calls; ranks are fixed functions of the row, so that they say which rows were handed over."""

    def __init__(self):
        self.calls, self.among_calls = [], []

    def rank_targets(self, seq, pos, max_item):
        self.calls.append((np.array(seq), np.array(pos), max_item))
        return (np.asarray(pos) % 23).astype(np.int32)

    def rank_targets_among(self, seq, pos, max_item, candidates=None, exclude_seen=False):
        self.among_calls.append((np.array(seq), np.array(pos), max_item, candidates, exclude_seen))
        return (np.asarray(pos) % 7).astype(np.int32)


class _OldStub:
    def rank_targets(self, seq, pos, max_item):
        return (np.asarray(pos) % 23).astype(np.int32)


def _sessions():
    rs = np.random.RandomState(3)
    return [rs.randint(1, 40, size=rs.randint(2, 9)).tolist() for _ in range(173)]


def _run(model, **kw):
    from ader_amd.data import Evaluator
    Evaluator.clear_cache()
    random.seed(21)
    ev = Evaluator(_sessions(), False, 10, 16, 40, "test", model, None, **kw)
    info = ev.evaluate(3)
    return ev, info, random.getstate()


def test_evaluator_calls_the_model_once_and_leaves_the_default_output_alone(capsys):
    from ader_amd.data import recall_mrr
    cand = [30, 2, 7, 7, 19]
    plain_model, model = _Stub(), _Stub()
    plain, plain_info, plain_state = _run(plain_model)
    plain_out = capsys.readouterr().out
    assert plain_model.among_calls == [] and len(plain_model.calls) == 1            # without the arguments: never called
    assert plain.ranks_among == []
    with pytest.raises(RuntimeError, match="candidates"):
        plain.results_among()

    ev, info, state = _run(model, candidates=cand, exclude_seen=True)
    out = capsys.readouterr().out
    assert len(model.calls) == 1 and len(model.among_calls) == 1
    seq, pos, max_item, c, ex = model.among_calls[0]
    assert np.array_equal(seq, model.calls[0][0]) and np.array_equal(pos, model.calls[0][1])      # the same concatenated rows
    assert len(pos) == len(ev.ranks) > 173 and max_item == 40 and c is cand and ex is True
    assert ev.ranks_among == (pos % 7).tolist() and ev.results_among() == recall_mrr(pos % 7)
    # evaluate() returns and prints what it did, and the `random` stream is where it was
    assert ev.ranks == plain.ranks and ev.results() == plain.results() and info == plain_info and out == plain_out
    assert state == plain_state
    line = ev.display_among(3)
    assert capsys.readouterr().out == line + "\n"
    assert line.startswith("epoch:3, test among 4 candidate items, seen items excluded (MRR@20: ") and ev.n_candidates() == 4

    only_seen, _, state2 = _run(_Stub(), exclude_seen=True)                         # no list: every item of 1..max_item
    assert only_seen.model.among_calls[0][3] is None and only_seen.model.among_calls[0][4] is True and state2 == plain_state
    assert only_seen.n_candidates() == 40 and "seen items excluded" in only_seen.display_among(1)


def test_evaluator_needs_a_model_with_the_method():
    with pytest.raises(RuntimeError, match="rank_targets_among"):
        _run(_OldStub(), candidates=[1, 2, 3])
    with pytest.raises(RuntimeError, match="rank_targets_among"):
        _run(_OldStub(), exclude_seen=True)
    ev, _, _ = _run(_OldStub())                                                     # the default needs nothing new
    assert len(ev.ranks) > 173
