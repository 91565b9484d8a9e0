"""Distillation from stored teacher representations (engine.TeacherRep, ader_teacher_rows), the parts that need no GPU: the launchers
are declared, bound, documented and exported; torch.ops.ader.teacher_rows traces under FakeTensorMode; the driver flag parses; an
ExemplarStore in the rep form round-trips through save / load."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ader_teacher_ranges", "ader_teacher_rows")


@pytest.fixture(scope="module")
def lib_path():
    from ader_amd import build
    return build.build()


def test_launchers_are_declared_bound_listed_and_exported(lib_path):
    import ctypes

    import torch  # noqa: F401  (one HIP runtime for the process, see ader_amd/_lib.py)
    from ader_amd import _lib
    header = open(os.path.join(ROOT, "include", "ader_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("## Exported symbols")[1].split("\n## ")[0]
    lib = ctypes.CDLL(lib_path)
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % n, header), n
        assert n in _lib.exported_symbols() and hasattr(lib, n), n
        assert "`%s`" % n in doc, n
    assert "util.py:433" in header.split("ader_teacher_ranges")[0].rsplit("/*", 1)[1]        # the TF sites it stands for
    assert "ADER.py:134-135" in header.split("ader_teacher_ranges")[0].rsplit("/*", 1)[1]
    assert len(_lib._SIGS["ader_teacher_rows"]) == 14
    # the step driver can replay it (a rep-form step stays plannable)
    _lib.load()
    assert _lib.step_fn_index("ader_teacher_rows") >= 0
    # ranges: a multiple of 8 (the block -> (range, chunk) mapping), at most ~one workgroup per CU over the chunks, and a workgroup
    # walks several tiles as soon as the catalog has more than 8 * 4 of them
    for Np, Bk in ((1, 64), (650, 64), (4097, 64), (4097, 192), (25750, 128), (1_000_000, 128), (1_000_000, 1024)):
        r = lib.ader_teacher_ranges(Np, Bk)
        tiles = (Np + 63) // 64
        assert r % 8 == 0 and r >= 8, (Np, Bk, r)
        assert r == 8 or r * (Bk // 64) <= 256, (Np, Bk, r)
        if tiles > 32:
            assert tiles / r > 2, (Np, Bk, r)
    # argument checks happen before anything is enqueued: each stated violation is -2 (no GPU is touched)
    ok = dict(n_ex=5, Bk=64, E=5, H=150, Np=33, ldr=36)
    for bad in (dict(H=161), dict(Bk=96), dict(n_ex=65), dict(Np=0), dict(ldr=32), dict(ldr=34)):
        a = dict(ok, **bad)
        rc = lib.ader_teacher_rows(None, None, None, a["n_ex"], a["Bk"], a["E"], a["H"], a["Np"], None, ctypes.c_long(a["ldr"]),
                                   None, None, None, None)
        assert rc == -2, (bad, rc)


def test_teacher_rows_traces_under_fake_tensors(lib_path):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    import ader_amd.ops  # noqa: F401
    with FakeTensorMode():
        trep, temb = torch.empty(90, 150), torch.empty(604, 150)
        rows, trl = torch.ops.ader.teacher_rows(trep, temb, torch.empty(37, dtype=torch.int32), 603)
        assert tuple(rows.shape) == (64, 603) and rows.dtype == torch.float32 and rows.stride(0) % 4 == 0 and rows.stride(1) == 1
        assert tuple(trl.shape) == (64,) and trl.dtype == torch.int32
        rows, trl = torch.ops.ader.teacher_rows(trep, temb, torch.empty(130, dtype=torch.int32), 64)
        assert tuple(rows.shape) == (192, 64) and tuple(trl.shape) == (192,)


def test_teacher_form_flag():
    from ader_amd.main import build_parser
    assert build_parser().parse_args([]).teacher_form == "logits"
    assert build_parser().parse_args(["--teacher_form", "rep"]).teacher_form == "rep"
    assert build_parser().parse_args(["--teacher_form", "logits"]).teacher_form == "logits"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--teacher_form", "bf16"])


def test_teacher_rep_record_checks_its_tensors():
    import torch
    from ader_amd.engine import TeacherRep
    rep, table = torch.randn(7, 12), torch.randn(34, 12)
    t = TeacherRep(rep, table, 33)
    assert len(t) == 7 and t.Np == 33 and t.nbytes() == (7 + 34) * 12 * 4
    with pytest.raises(RuntimeError):
        TeacherRep(rep.double(), table, 33)                    # dtype
    with pytest.raises(RuntimeError):
        TeacherRep(rep, torch.randn(12, 34).t(), 33)           # a non-contiguous table
    with pytest.raises(RuntimeError):
        TeacherRep(rep, table, 34)                             # the snapshot has no row for item 34
    with pytest.raises(RuntimeError):
        TeacherRep(rep, torch.randn(34, 16), 33)               # H differs
    with pytest.raises(RuntimeError):
        t.rows([0])                                            # CPU tensors: no fallback


def test_store_in_rep_form_round_trips(tmp_path):
    import torch
    from ader_amd.engine import TeacherRep
    from ader_amd.exemplar import ExemplarStore
    g = torch.Generator().manual_seed(3)
    E, T, H, Np = 9, 20, 12, 33
    rows = np.random.RandomState(0).randint(0, Np + 1, size=(E, T + 1)).astype(np.int32)
    rep, table = torch.randn(E, H, generator=g), torch.randn(Np + 1, H, generator=g)
    st = ExemplarStore(rows, TeacherRep(rep, table, Np), Np)
    assert st.form == "rep" and len(st) == E
    assert sum(np.asarray(t).nbytes if not hasattr(t, "element_size") else t.numel() * t.element_size() for t in st.tensors()) \
        == E * H * 4 + (Np + 1) * H * 4 + rows.nbytes
    path = st.save(str(tmp_path / "exemplars.pt"))
    back = ExemplarStore.load(path)
    assert back.form == "rep" and back.max_item == Np and back.teacher.Np == Np
    assert np.array_equal(back.rows, rows) and back.rows.dtype == np.int32
    assert back.teacher.rep.numpy().tobytes() == rep.numpy().tobytes()
    assert back.teacher.table.numpy().tobytes() == table.numpy().tobytes()
    assert back.sessions()[0] == st.sessions()[0]
    # the dense form still round-trips as before, and says what it is
    dense = ExemplarStore(rows, torch.randn(E, Np, generator=g), Np)
    back_d = ExemplarStore.load(dense.save(str(tmp_path / "dense.pt")))
    assert dense.form == back_d.form == "logits" and back_d.logits.numpy().tobytes() == dense.logits.numpy().tobytes()
