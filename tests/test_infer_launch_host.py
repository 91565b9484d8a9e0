"""Host checks of the inference launch layer (ader_amd/engine/infer_launch.py): every launch function's launcher and argument list
against the prototypes of include/ader_hip.h and the ctypes table, the padded ncol / target stages, the NULL rules of the lists and of
seen, and the scratch sizes the header states.  No GPU: the tensors live on the CPU, the launcher call is replaced by a recorder, and
only the pure host size queries reach the real library."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_table_job_host import param_names  # noqa: E402

from ader_amd import _lib  # noqa: E402
from ader_amd.engine import infer_launch as L  # noqa: E402

H, ITEMS, N, K, M, C, S = 16, 300, 280, 5, 130, 70, 8
WIDE_K, WIDE_CAP, BAND, X3_CAP = 70, 192, 16, 4096
STREAM, EMB = 0x5151, 0x7E000000                                # (emb travels as an address)
QUERIES = {"ader_topk_kmax", "ader_topk_ranges", "ader_topk_rows_ranges", "ader_row_stats_floats", "ader_topk_x3_ranges",
           "ader_topk_x3_kmax", "ader_topk_wide_kmax", "ader_topk_wide_cap", "ader_topk_wide_slabs"}
I32, I64, F32, BF16 = torch.int32, torch.int64, torch.float32, torch.bfloat16


def query(name, *args):
    return _lib.call(name, *args)


class Ws:
    """A persistent allocator keyed by name, as Engine.buf: the same tensor again for the same name, shape and dtype."""

    def __init__(self):
        self.held = {}

    def __call__(self, name, shape, dtype=F32):
        assert isinstance(shape, tuple), name
        t = self.held.get(name)
        if t is None or t.shape != shape or t.dtype != dtype:
            t = self.held[name] = torch.full(shape, 77, dtype=dtype)      # (stale contents: a stage that is not cleared shows)
        return t


class Scratch:
    """Expected: a buffer the launch function took from ws, of this dtype and at least this many elements; `head` = (B, values) checks
    [:B] == values and [B:] == 0."""

    def __init__(self, dtype, numel, head=None):
        self.dtype, self.numel, self.head = dtype, numel, head


@pytest.fixture
def calls(monkeypatch):
    got = []
    monkeypatch.setattr(L, "call", lambda name, *a: query(name, *a) if name in QUERIES else got.append((name, a)))
    return got


def inputs(B, k=K, lists="given"):
    """Distinct CPU tensors for every role of one call."""
    z = lambda *s, dt=I32: torch.zeros(s, dtype=dt)                 # noqa: E731
    m, c = (M, C) if lists == "given" else (0, 0)
    return dict(rep=z(B, H, dt=F32), target=torch.arange(1, B + 1, dtype=I32), seen=z(B, S), status=z(1), emax=z(1, dt=F32),
                cand=None if lists == "none" else z(m), ids=None if lists == "none" else z(B, c), items=z(B, k), scores=z(B, k, dt=F32),
                lse=z(B, dt=F32), entropy=z(B, dt=F32), out=z(B, N + 4, dt=F32)[:, :N], list_scores=z(B, c, dt=F32),
                diag=z(8), m=m, c=c)


def p(t):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def stages(B, Bp, t, target=False):
    w = {"ncol": Scratch(I32, Bp, (B, N))}
    if target:
        w.update(target=Scratch(I32, Bp, (B, t["target"])), tlogit=Scratch(F32, Bp), rank=Scratch(I32, Bp))
    return w


def seen_of(t, seen):
    return {"seen": p(t["seen"]) if seen else None, "seen_ld": S if seen else 0}


# case -> (launcher, row padding, run(ws, t, seen) -> what the function returned, want(B, Bp, t, seen) -> expected by parameter name,
#          names of the parameters whose buffers the function returns, in order)
def _logits_store():
    return ("ader_logits_store", 64, lambda ws, t, s: L.logits_store(ws, STREAM, t["rep"], EMB, H, N, t["out"]),
            lambda B, Bp, t, s: {"ncol_all": Scratch(I32, Bp, (B, N)), "out": p(t["out"]), "ldo": N + 4}, ())


def _rank_targets():
    return ("ader_rank_targets", 64, lambda ws, t, s: L.rank_targets(ws, STREAM, t["rep"], EMB, H, N, t["target"]),
            lambda B, Bp, t, s: stages(B, Bp, t, True), ("rank",))


def _rank_targets_x3(own_diag):
    def run(ws, t, s):
        return L.rank_targets_x3(ws, STREAM, t["rep"], EMB, ITEMS, H, N, t["target"], t["emax"], X3_CAP, t["diag"] if own_diag else None)

    def want(B, Bp, t, s):
        return dict(stages(B, Bp, t, True), item_num=ITEMS, rep_hi=Scratch(BF16, Bp * 168), rep_lo=Scratch(BF16, Bp * 168),
                    delta=Scratch(F32, Bp), emax=p(t["emax"]), cand=Scratch(I32, 3 * X3_CAP), cap=X3_CAP,
                    diag=p(t["diag"]) if own_diag else Scratch(I32, 2))
    return "ader_rank_targets_x3", 128, run, want, ("rank", "diag")


def _rank_targets_cand():
    def run(ws, t, s):
        return L.rank_targets_cand(ws, STREAM, t["rep"], EMB, H, N, t["target"], t["cand"], t["seen"] if s else None, t["status"])
    return ("ader_rank_targets_cand", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t, True), cand=p(t["cand"]), M=t["m"], status=p(t["status"]), **seen_of(t, s)), ("rank",))


def _rank_targets_rows():
    def run(ws, t, s):
        return L.rank_targets_rows(ws, STREAM, t["rep"], EMB, H, N, t["target"], t["ids"], t["seen"] if s else None, t["status"])
    return ("ader_rank_targets_rows", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t, True), ids=p(t["ids"]), ld=t["c"], C=t["c"], status=p(t["status"]), **seen_of(t, s)),
            ("rank",))


def answer(t):
    return {"items": p(t["items"]), "scores": p(t["scores"])}


def _topk_items():
    def run(ws, t, s):
        return L.topk_items(ws, STREAM, t["rep"], EMB, H, N, t["seen"] if s else None, K, t["items"], t["scores"])
    return ("ader_topk_items", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t), k=K, part=Scratch(I64, query("ader_topk_ranges", N, Bp) * Bp * K), **answer(t),
                                     **seen_of(t, s)), ())


def _topk_items_cand():
    def run(ws, t, s):
        return L.topk_items_cand(ws, STREAM, t["rep"], EMB, H, N, t["cand"], t["seen"] if s else None, K, t["items"], t["scores"], t["status"])
    return ("ader_topk_items_cand", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t), cand=p(t["cand"]), M=t["m"], k=K, status=p(t["status"]),
                                     part=Scratch(I64, query("ader_topk_ranges", t["m"], Bp) * Bp * K), **answer(t), **seen_of(t, s)), ())


def _topk_items_rows():
    def run(ws, t, s):
        return L.topk_items_rows(ws, STREAM, t["rep"], EMB, H, N, t["ids"], t["seen"] if s else None, K, t["items"], t["scores"], t["status"])
    return ("ader_topk_items_rows", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t), ids=p(t["ids"]), ld=t["c"], C=t["c"], k=K, status=p(t["status"]),
                                     part=Scratch(I64, query("ader_topk_rows_ranges", t["c"], K) * Bp * K), **answer(t), **seen_of(t, s)), ())


def _topk_items_x3(own_diag):
    def run(ws, t, s):
        return L.topk_items_x3(ws, STREAM, t["rep"], EMB, ITEMS, H, N, t["seen"] if s else None, K, BAND, t["emax"], t["items"], t["scores"],
                               t["diag"] if own_diag else None)

    def want(B, Bp, t, s):
        return dict(stages(B, Bp, t), item_num=ITEMS, k=K, band=BAND, rep_hi=Scratch(BF16, Bp * 168), rep_lo=Scratch(BF16, Bp * 168),
                    delta=Scratch(F32, Bp), emax=p(t["emax"]), part3=Scratch(I64, query("ader_topk_x3_ranges", N, Bp) * Bp * (K + BAND)),
                    status=Scratch(I32, Bp), diag=p(t["diag"]) if own_diag else Scratch(I32, 3), **answer(t), **seen_of(t, s))
    return "ader_topk_items_x3", 128, run, want, ("status", "diag")


def _topk_items_wide(own_diag):
    def run(ws, t, s):
        return L.topk_items_wide(ws, STREAM, t["rep"], EMB, H, N, t["seen"] if s else None, WIDE_K, WIDE_CAP, t["items"], t["scores"],
                                 t["diag"] if own_diag else None)

    def want(B, Bp, t, s):
        return dict(stages(B, Bp, t), k=WIDE_K, cap=WIDE_CAP, list=Scratch(I64, Bp * WIDE_CAP), cnt=Scratch(I32, Bp), thr=Scratch(I64, Bp),
                    row_status=Scratch(I32, Bp), diag=p(t["diag"]) if own_diag else Scratch(I32, 2), **answer(t), **seen_of(t, s))
    return "ader_topk_items_wide", 64, run, want, ("row_status", "diag")


def stats(t):
    return {"lse": p(t["lse"]), "entropy": p(t["entropy"])}


def _row_stats():
    return ("ader_row_stats", 64, lambda ws, t, s: L.row_stats(ws, STREAM, t["rep"], EMB, H, N, t["lse"], t["entropy"]),
            lambda B, Bp, t, s: dict(stages(B, Bp, t), spart=Scratch(F32, query("ader_row_stats_floats", N, Bp)), **stats(t)), ())


def _topk_items_stats():
    def run(ws, t, s):
        return L.topk_items_stats(ws, STREAM, t["rep"], EMB, H, N, t["seen"] if s else None, K, t["items"], t["scores"], t["lse"],
                                  t["entropy"])
    return ("ader_topk_items_stats", 64, run,
            lambda B, Bp, t, s: dict(stages(B, Bp, t), k=K, part=Scratch(I64, query("ader_topk_ranges", N, Bp) * Bp * K),
                                     spart=Scratch(F32, query("ader_row_stats_floats", N, Bp)), **answer(t), **stats(t), **seen_of(t, s)), ())


CASES = {
    "logits_store": _logits_store(), "rank_targets": _rank_targets(), "rank_targets_x3": _rank_targets_x3(False),
    "rank_targets_x3, caller's diag": _rank_targets_x3(True), "rank_targets_cand": _rank_targets_cand(),
    "rank_targets_rows": _rank_targets_rows(), "topk_items": _topk_items(), "topk_items_cand": _topk_items_cand(),
    "topk_items_rows": _topk_items_rows(), "topk_items_x3": _topk_items_x3(False), "topk_items_x3, caller's diag": _topk_items_x3(True),
    "topk_items_wide": _topk_items_wide(False), "topk_items_wide, caller's diag": _topk_items_wide(True), "row_stats": _row_stats(),
    "topk_items_stats": _topk_items_stats(),
}
WITH_LISTS = ("rank_targets_cand", "rank_targets_rows", "topk_items_cand", "topk_items_rows")


def check_call(name, args, want, ws, returned, returns):
    sig, names = _lib._SIGS[name], param_names(name)
    assert len(args) == len(sig) == len(names)
    for a, ty, n in zip(args, sig, names):
        if ty is _lib.P:
            assert a is None or type(a) is int, n
        else:
            assert ty in (_lib.I, _lib.L) and type(a) is int, n
    got = dict(zip(names, args))
    assert set(want) == set(names), set(want) ^ set(names)          # every slot of the prototype is checked by name
    ptrs = [a for a, ty in zip(args, sig) if ty is _lib.P and a is not None and a != STREAM]
    assert len(set(ptrs)) == len(ptrs), "one buffer for two parameters of %s" % name
    held = {t.data_ptr(): t for t in ws.held.values()}
    for n, w in want.items():
        if not isinstance(w, Scratch):
            assert got[n] == w, n
            continue
        t = held.get(got[n])
        assert t is not None, "%s is not a workspace buffer" % n
        assert t.dtype == w.dtype and t.numel() >= w.numel, (n, t.dtype, t.numel(), w.numel)
        if w.head is not None:
            B, values = w.head
            assert torch.equal(t[:B], torch.zeros(B, dtype=I32) + values) and not t[B:].any(), n
    returned = () if returned is None else returned if isinstance(returned, tuple) else (returned,)
    assert [r.data_ptr() for r in returned] == [got[n] for n in returns]


def run_case(case, B, seen, lists, calls, ws):
    launcher, pad, run, want, returns = CASES[case]
    t = inputs(B, WIDE_K if "wide" in case else K, lists)
    del calls[:]
    returned = run(ws, t, seen)
    assert len(calls) == 1 and calls[0][0] == launcher
    Bp = (B + pad - 1) // pad * pad
    assert Bp == {(70, 64): 128, (70, 128): 128, (64, 64): 64, (64, 128): 128}[B, pad]
    w = dict(want(B, Bp, t, seen), rep=p(t["rep"]), emb=EMB, B=B, Bp=Bp, H=H, N=N, stream=STREAM)
    check_call(launcher, calls[0][1], w, ws, returned, returns)


@pytest.mark.parametrize("seen", [True, False], ids=["seen", "seen NULL"])
@pytest.mark.parametrize("B", [70, 64])
@pytest.mark.parametrize("case", sorted(CASES))
def test_marshalling(case, B, seen, calls):
    run_case(case, B, seen, "given", calls, Ws())


@pytest.mark.parametrize("lists", ["empty", "none"])
@pytest.mark.parametrize("case", WITH_LISTS)
def test_an_empty_list_is_null(case, lists, calls):
    run_case(case, 70, True, lists, calls, Ws())
    got = dict(zip(param_names(CASES[case][0]), calls[0][1]))
    assert (got["cand"], got["M"]) == (None, 0) if "cand" in case else (got["ids"], got["ld"], got["C"]) == (None, 0, 0)


@pytest.mark.parametrize("B", [70, 64])
def test_score_items(B, calls):
    """No padded stage: Bp = B, ncol = NULL, no workspace (seen is not a parameter of this launcher)."""
    for lists in ("given", "empty", "none"):
        t = inputs(B, lists=lists)
        del calls[:]
        assert L.score_items(STREAM, t["rep"], EMB, H, N, t["ids"], t["list_scores"]) is None
        assert len(calls) == 1 and calls[0][0] == "ader_score_items"
        want = dict(rep=p(t["rep"]), emb=EMB, B=B, H=H, N=N, ncol=None, ids=p(t["ids"]), ld=t["c"], C=t["c"], scores=t["list_scores"].data_ptr(),
                    ld_scores=t["c"], stream=STREAM)
        check_call("ader_score_items", calls[0][1], want, Ws(), None, ())


def test_rank_emax(calls):
    ws = Ws()
    emax = L.rank_emax(ws, STREAM, EMB, ITEMS, H, N)
    assert len(calls) == 1 and calls[0][0] == "ader_rank_emax"
    check_call("ader_rank_emax", calls[0][1], dict(emb=EMB, item_num=ITEMS, H=H, N=N, emax=Scratch(F32, 1), stream=STREAM), ws, emax, ("emax",))


@pytest.mark.parametrize("order", ["forward", "backward"])
def test_a_persistent_workspace_never_serves_two_parameters_of_one_call(order, calls):
    """One allocator across all launch functions in turn, as Engine.buf serves them: check_call finds every pointer of a call distinct,
    with emax -- rank_emax's buffer of the same workspace -- among them."""
    ws = Ws()
    names = sorted(CASES) if order == "forward" else sorted(CASES, reverse=True)
    for B in (70, 64):
        for case in names + names:
            launcher, pad, run, want, returns = CASES[case]
            t = inputs(B, WIDE_K if "wide" in case else K)
            del calls[:]
            t["emax"] = L.rank_emax(ws, STREAM, EMB, ITEMS, H, N)
            del calls[:]
            returned = run(ws, t, True)
            Bp = (B + pad - 1) // pad * pad
            w = dict(want(B, Bp, t, True), rep=p(t["rep"]), emb=EMB, B=B, Bp=Bp, H=H, N=N, stream=STREAM)
            check_call(launcher, calls[0][1], w, ws, returned, returns)


def test_every_launcher_called_by_the_layer_has_a_row_here():
    src = open(L.__file__).read()
    called = set(re.findall(r'call\("(ader_[a-z0-9_]+)"', src)) - QUERIES
    assert called == {c[0] for c in CASES.values()} | {"ader_rank_emax", "ader_score_items"}
