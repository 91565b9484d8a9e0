"""Distilling from a TeacherRep on the catalog-sharded table (TeacherRep.lse, ader_teacher_rows_shard, common.teacher_window), the
parts that need no GPU: the record checks and carries its log-sum-exps, the store writes and reads them, the overlapping window view
addresses a rank's block by global column inside its allocation, the launcher is declared, bound, documented and exported and refuses
what it states, the operator traces under FakeTensorMode, the refusal names the way out, and the generator asks for the log-sum-exps
exactly when its engine steps catalog-sharded."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ader_teacher_rows_shard"


@pytest.fixture(scope="module")
def lib_path():
    from ader_amd import build
    return build.build()


# ------------------------------------------------------------------------------------------------------------- the record
def test_record_checks_and_carries_its_lse():
    from ader_amd.engine import TeacherRep
    rep, table = torch.randn(7, 12), torch.randn(34, 12)
    lse = torch.randn(7)
    t = TeacherRep(rep, table, 33, lse)
    assert t.lse is lse and len(t) == 7
    assert t.nbytes() == (7 + 34) * 12 * 4 + 7 * 4
    assert TeacherRep(rep, table, 33).lse is None and TeacherRep(rep, table, 33).nbytes() == (7 + 34) * 12 * 4
    for bad in (lse.double(),                       # dtype
                torch.randn(8), torch.randn(7, 1),  # shape [E]
                torch.randn(14)[::2],               # contiguity
                torch.empty(7, device="meta"),      # another device than rep's
                lse.numpy()):                       # no tensor
        with pytest.raises(RuntimeError, match="lse"):
            TeacherRep(rep, table, 33, bad)
    moved = t.to("cpu")
    assert moved.lse is not None and moved.lse.numpy().tobytes() == lse.numpy().tobytes() and moved.Np == 33
    assert TeacherRep(rep, table, 33).to("cpu").lse is None
    meta = t.to("meta")                            # every tensor of the record moves, lse included
    assert meta.lse.device.type == "meta" and meta.rep.device.type == "meta" and tuple(meta.lse.shape) == (7,)


def test_key_of_a_record_without_lse_is_unchanged():
    from ader_amd.engine import TeacherRep
    rep, table = torch.randn(7, 12), torch.randn(34, 12)
    t = TeacherRep(rep, table, 33)
    assert t.key() == ("rep", rep.data_ptr(), (7, 12), table.data_ptr(), (34, 12), 33)


# ------------------------------------------------------------------------------------------------------------- the store
def test_store_round_trips_with_and_without_lse(tmp_path):
    from ader_amd.engine import TeacherRep
    from ader_amd.exemplar import ExemplarStore
    g = torch.Generator().manual_seed(5)
    E, T, H, Np = 9, 20, 12, 33
    rows = np.random.RandomState(1).randint(0, Np + 1, size=(E, T + 1)).astype(np.int32)
    rep, table, lse = torch.randn(E, H, generator=g), torch.randn(Np + 1, H, generator=g), torch.randn(E, generator=g)
    st = ExemplarStore(rows, TeacherRep(rep, table, Np, lse), Np)
    assert st.form == "rep" and any(x is lse for x in st.tensors())
    back = ExemplarStore.load(st.save(str(tmp_path / "with.pt")))
    assert back.form == "rep" and back.teacher.Np == Np and np.array_equal(back.rows, rows)
    assert back.teacher.lse.dtype == torch.float32 and back.teacher.lse.numpy().tobytes() == lse.numpy().tobytes()
    assert back.teacher.rep.numpy().tobytes() == rep.numpy().tobytes()
    assert back.teacher.table.numpy().tobytes() == table.numpy().tobytes()
    # without: no entry is written, and the record comes back without
    st0 = ExemplarStore(rows, TeacherRep(rep, table, Np), Np)
    assert len(st0.tensors()) == 3
    p0 = st0.save(str(tmp_path / "without.pt"))
    assert "lse" not in torch.load(p0, weights_only=True)
    assert ExemplarStore.load(p0).teacher.lse is None
    # a file of the earlier layout (exactly these five entries)
    old = str(tmp_path / "old.pt")
    torch.save({"rows": torch.from_numpy(rows), "rep": rep, "table": table, "Np": Np, "max_item": Np}, old)
    b = ExemplarStore.load(old)
    assert b.teacher.lse is None and b.teacher.rep.numpy().tobytes() == rep.numpy().tobytes() and b.max_item == Np


# ------------------------------------------------------------------------------------------------------------- the window
@pytest.mark.parametrize("W", range(1, 9))
def test_window_view_addresses_the_block_by_global_column(W):
    from ader_amd.engine.common import teacher_window, teacher_window_numel
    S, n_rows = 128, 2 * W                          # (the helper does not care what a row is: two rows per rank keep this small)
    for r in range(W):
        ib = r * S
        n = teacher_window_numel(n_rows, ib, S)
        assert n == ib + n_rows * S
        buf = torch.arange(n, dtype=torch.float32)
        view, block = teacher_window(buf, n_rows, ib, S)
        assert tuple(view.shape) == (n_rows, ib + S) and view.stride() == (S, 1) and tuple(block.shape) == (n_rows, S)
        assert view.data_ptr() == buf.data_ptr() and block.data_ptr() == buf.data_ptr() + 4 * ib and block.stride() == (S, 1)
        # view[t, ib + c] IS block[t, c]: the same element of buf
        idx = ib + torch.arange(n_rows)[:, None] * S + torch.arange(S)[None, :]
        assert torch.equal(block, idx.float()) and torch.equal(view[:, ib:], block)
        for t in (0, n_rows - 1):
            for c in (0, S - 1):
                assert view[t, ib + c].data_ptr() == block[t, c].data_ptr() == buf.data_ptr() + 4 * (ib + t * S + c)
        # the dummy column 0 of every row and the view's last element lie inside the allocation
        assert all(0 <= (view[t, 0].data_ptr() - buf.data_ptr()) // 4 == t * S < n for t in range(n_rows))
        assert (view[n_rows - 1, ib + S - 1].data_ptr() - buf.data_ptr()) // 4 == n - 1
        # the blocks of different rows do not overlap: a row written through the block changes no other row's block
        buf.zero_()
        for t in range(n_rows):
            block[t].fill_(t + 1.0)
        assert torch.equal(block, (torch.arange(n_rows, dtype=torch.float32) + 1)[:, None].expand(n_rows, S))
        assert torch.equal(buf[:ib], torch.zeros(ib))                                  # nothing left of the window is a block
    for bad in (dict(item_begin=2), dict(S=192), dict(numel=-1), dict(n_rows=0)):
        a = dict(dict(n_rows=4, item_begin=128, S=128, numel=0), **bad)
        with pytest.raises(RuntimeError):
            teacher_window(torch.zeros(teacher_window_numel(max(a["n_rows"], 1), a["item_begin"], a["S"]) + a["numel"]),
                           a["n_rows"], a["item_begin"], a["S"])


# ------------------------------------------------------------------------------------------------------------- the launcher
def test_launcher_is_declared_bound_listed_exported_and_refuses_what_it_states(lib_path):
    from ader_amd import _lib
    header = open(os.path.join(ROOT, "include", "ader_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    listed = doc.split("## Exported symbols")[1].split("\n## ")[0]
    lib = ctypes.CDLL(lib_path)
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in _lib.exported_symbols() and hasattr(lib, NAME) and "`%s`" % NAME in listed
    assert "lib.%s.argtypes" % NAME in doc
    comment = header.split("int " + NAME)[0].rsplit("/*", 1)[1]
    assert "util.py:433" in comment and "ADER.py:134-135" in comment                   # the TF sites it stands for
    assert len(_lib._SIGS[NAME]) == 15
    fn = getattr(lib, NAME)
    fn.argtypes = _lib._SIGS[NAME]
    ok = dict(n_ex=70, Bk=128, E=70, H=150, Np=700, ib=384, ic=384, ldr=384)
    # argument checks happen before anything is enqueued: each stated violation is -2 (no GPU is touched)
    for bad in (dict(ib=386), dict(ib=-4), dict(ic=-1), dict(ldr=382), dict(ldr=312),       # 316 items: ldr < n_loc
                dict(H=161), dict(H=0), dict(Bk=96), dict(n_ex=129), dict(Np=0)):
        a = dict(ok, **bad)
        rc = fn(None, None, None, a["n_ex"], a["Bk"], a["E"], a["H"], a["Np"], a["ib"], a["ic"], None, a["ldr"], None, None, None)
        assert rc == -2, (bad, rc)


def test_operator_traces_under_fake_tensors(lib_path):
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        trep, temb = torch.empty(70, 150), torch.empty(701, 150)
        ex = torch.empty(37, dtype=torch.int32)
        for Np, ib, ic, n_loc in ((700, 0, 384, 384), (700, 384, 384, 316), (650, 384, 384, 266), (530, 512, 256, 18), (500, 512, 256, 0)):
            rows, trl = torch.ops.ader.teacher_rows_shard(trep, temb, ex, Np, ib, ic)
            assert tuple(rows.shape) == (64, n_loc) and rows.dtype == torch.float32
            assert n_loc == 0 or (rows.stride(0) % 4 == 0 and rows.stride(0) >= n_loc and rows.stride(1) == 1)
            assert tuple(trl.shape) == (64,) and trl.dtype == torch.int32


# ------------------------------------------------------------------------------------------------------------- engine and generator
class _Eng:
    """What Engine._check_teacher and ExemplarGenerator._make_store read of an engine."""

    def __init__(self, world, mode):
        self.dp_world, self.dp_mode, self.asked = world, mode, []

    def teacher_rep(self, seq, max_item, **kw):
        self.asked.append(("rep", kw))
        return "rep-record"

    def teacher_logits(self, seq, max_item):
        self.asked.append(("logits", {}))
        return "logits"


def test_refusal_only_without_lse_and_names_the_way_out():
    from ader_amd.engine import Engine, TeacherRep
    rep, table = torch.randn(7, 12), torch.randn(34, 12)
    bare, full = TeacherRep(rep, table, 33), TeacherRep(rep, table, 33, torch.randn(7))
    with pytest.raises(RuntimeError, match=r"catalog.*teacher_rep\(\.\.\., lse=True\)"):
        Engine._check_teacher(_Eng(2, "catalog"), bare)
    Engine._check_teacher(_Eng(2, "catalog"), full)
    Engine._check_teacher(_Eng(2, "catalog"), torch.randn(7, 33))
    Engine._check_teacher(_Eng(2, "catalog"), None)
    Engine._check_teacher(_Eng(2, "replicated"), bare)
    Engine._check_teacher(_Eng(1, "catalog"), bare)


def test_generator_asks_for_lse_exactly_when_the_engine_steps_catalog_sharded():
    from ader_amd.exemplar import ExemplarGenerator

    class _Model:
        pass

    rows = np.zeros((3, 21), dtype=np.int32)
    for world, mode, form, want in ((2, "catalog", "rep", ("rep", {"lse": True})), (2, "replicated", "rep", ("rep", {})),
                                    (1, "catalog", "rep", ("rep", {})), (2, "catalog", "logits", ("logits", {}))):
        gen = ExemplarGenerator.__new__(ExemplarGenerator)
        gen.teacher_form, gen.maxlen, gen.max_item = form, 20, 33
        m = _Model()
        m.engine = _Eng(world, mode)
        gen._make_store(m, rows)
        assert m.engine.asked == [want], (world, mode, form, m.engine.asked)
