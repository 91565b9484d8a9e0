"""Host checks of the fused table update's issue path (engine/common.py: TableJob, issue_table_job, flash_sizes): every form's
launcher and argument list against the prototypes of include/ader_hip.h and the ctypes table, and the flash-loss layout constants
against the kernel headers.  No GPU: the records are built from CPU tensors and the launcher call is replaced by a recorder."""
import os
import re

import numpy as np
import pytest
import torch

from ader_amd import _lib
from ader_amd.engine import common
from ader_amd.engine.common import HP, LDR, PART_LD, X3_IMG_ROW_B, TableJob, flash_sizes, issue_table_job

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, ITEMS, N, NP = 6, 300, 280, 200
BT, BK = 128, 128
B1, B2, EPS, LR_T = 0.9, 0.999, 1e-8, 3e-4
STREAM = 0x5151


def param_names(launcher):
    """Parameter names of a launcher, in order, from its prototype in include/ader_hip.h."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ader_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % re.escape(launcher), src, flags=re.S)
    assert m, launcher
    return [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)[-1] for p in m.group(1).split(",")]


def make(x3, kd=False, extra=False):
    """(record, lists, table, shadow, rep_img) over distinct CPU tensors."""
    Bp = BT + BK if kd else BT
    f, i = torch.zeros, lambda n: torch.zeros(n, dtype=torch.int32)       # noqa: E731
    n_sp = 7 * Bp
    job = TableJob(f(Bp * LDR, dtype=torch.bfloat16), f(Bp * LDR, dtype=torch.bfloat16) if x3 else None, Bp if kd else 100, Bp, N,
                   f(Bp), i(Bp), f(Bp), f(n_sp, H), i(n_sp), f(ITEMS + 1, H) if extra else None)
    if kd:
        job.kd_row0, job.Np, job.teacher, job.trow, job.tlse2 = BT, NP, f(40, NP + 8)[:, :NP], i(Bp), f(Bp)
    lists = (i(n_sp), i(n_sp), i(9), i(Bp), i(Bp), i(9), i(64))           # ids, order, sp_start, tids, torder, tg_start, meta
    table = tuple(f(ITEMS + 1, H) for _ in range(3))
    shadow = None if x3 else f((ITEMS + 1) * LDR, dtype=torch.bfloat16)
    img = f(Bp * X3_IMG_ROW_B, dtype=torch.uint8) if x3 else None
    return job, lists, table, shadow, img


# form -> (x3, distilled, extra, (tile_begin, tile_count) or None, bf16 form, launcher)
FORMS = {
    "x3": (True, False, False, None, "sh", "ader_tab_update_x3"),
    "x3+extra": (True, False, True, None, "sh", "ader_tab_update_x3"),
    "x3 distilled": (True, True, False, None, "sh", "ader_tab_update_x3_kd"),
    "x3 distilled, tile range": (True, True, False, (2, 1), "sh", "ader_tab_update_x3_kd_range"),
    "x3, tile range": (True, False, False, (1, 2), "sh", "ader_tab_update_x3"),
    "sh": (False, False, False, None, "sh", "ader_tab_update_sh"),
    "sh, tile range": (False, False, False, (1, 2), "sh", "ader_tab_update_sh"),
    "sh distilled": (False, True, False, None, "sh", "ader_tab_update_sh_kd"),
    "resident": (False, False, False, None, "resident", "ader_tab_update"),
}


@pytest.fixture
def calls(monkeypatch):
    got = []
    monkeypatch.setattr(common, "call", lambda name, *args: got.append((name, args)))
    return got


def issue(job, lists, table, shadow, img, tiles=None, bf16="sh"):
    kw = {} if tiles is None else dict(tile_begin=tiles[0], tile_count=tiles[1])
    issue_table_job(job, lists, table, ITEMS, H, shadow, img, LR_T, B1, B2, EPS, STREAM, bf16=bf16, **kw)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_marshalling(form, calls):
    x3, kd, extra, tiles, bf16, launcher = FORMS[form]
    job, lists, table, shadow, img = make(x3, kd, extra)
    issue(job, lists, table, shadow, img, tiles, bf16)
    assert len(calls) == 1
    name, args = calls[0]
    assert name == launcher
    sig = (_lib._XSIGS if name == "ader_tab_update" else _lib._SIGS)[name]
    names = param_names(name)
    assert len(args) == len(sig) == len(names)
    for a, t, n in zip(args, sig, names):
        if t is _lib.P:
            assert a is None or type(a) is int, n
        elif t is _lib.F:
            assert isinstance(a, float), n
        else:
            assert t in (_lib.I, _lib.L) and type(a) is int, n
    got = dict(zip(names, args))
    ids, order, sp_start, tids, torder, tg_start, meta = lists
    want = {"rep_hi" if "rep_hi" in got else "rep_bf": job.hi.data_ptr(), "item_num": ITEMS, "Bp": job.Bp, "H": H, "N": N,
            "off": job.off.data_ptr(), "wrow": job.wrow.data_ptr(), "sp_src": job.g.data_ptr(), "sp_ids": ids.data_ptr(),
            "sp_rows": order.data_ptr(), "tg_ids": tids.data_ptr(), "tg_rows": torder.data_ptr(), "n_sp": ids.numel(),
            "n_tg": tids.numel(), "sp_scale": float(np.sqrt(np.float32(H))), "emb": table[0].data_ptr(),
            "adam_m": table[1].data_ptr(), "adam_v": table[2].data_ptr(), "lr_t": LR_T, "beta1": B1, "beta2": B2, "eps": EPS,
            "stream": STREAM}
    if x3:
        want.update(rep_lo=job.lo.data_ptr(), rep_img=img.data_ptr(), tile_meta=meta.data_ptr())
    else:
        want["shadow"] = shadow.data_ptr()
        if bf16 == "resident":
            want["tile_meta"] = meta.data_ptr()
        else:
            want.update(sp_start=sp_start.data_ptr(), tg_start=tg_start.data_ptr())
    if kd:
        want.update(kd_row0=BT, Np=NP, teacher=job.teacher.data_ptr(), ldt=NP + 8, trow=job.trow.data_ptr(),
                    tlse2=job.tlse2.data_ptr())
    else:
        want.update(B=job.B, extra_grad=job.extra.data_ptr() if extra else None)
    if not kd or tiles is not None:
        want.update(tile_begin=tiles[0] if tiles else 0, tile_count=tiles[1] if tiles else -1)
    assert set(want) == set(names), set(want) ^ set(names)      # every slot of the prototype is checked by name
    assert got == want


def test_planted_faults_raise_before_the_launch(calls):
    job, lists, table, shadow, img = make(True, kd=True)
    job.teacher = None                                          # kd_row0 set, no teacher
    with pytest.raises(RuntimeError):
        issue(job, lists, table, shadow, img)
    job, lists, table, shadow, img = make(True, kd=True, extra=True)
    with pytest.raises(RuntimeError):                           # a tile range together with `extra` on a distilled job
        issue(job, lists, table, shadow, img, tiles=(0, 2))
    job, lists, table, shadow, img = make(False, kd=True)
    with pytest.raises(RuntimeError):                           # no launcher: distilled bf16 update with a tile range
        issue(job, lists, table, shadow, img, tiles=(0, 2))
    assert calls == []


def defines(path, names):
    src = open(os.path.join(ROOT, "ader_amd", "csrc", path)).read()
    return {n: int(re.search(r"^#define\s+%s\s+(\d+)\b" % n, src, flags=re.M).group(1)) for n in names}


def test_layout_constants_match_the_kernel_headers():
    assert defines("lbf_common.h", ("LDR", "HP")) == {"LDR": LDR, "HP": HP}
    assert defines("seq_common.h", ("LDR", "HP")) == {"LDR": LDR, "HP": HP}
    assert defines("logits_bf16.hip", ("PART_LD",)) == {"PART_LD": PART_LD}
    assert defines("x3_image.h", ("X3_IMG_B",))["X3_IMG_B"] == 32 * X3_IMG_ROW_B
    assert (LDR, HP, PART_LD, X3_IMG_ROW_B) == (168, 160, 152, 704)


@pytest.mark.parametrize("R,Bp,R2,Bk", [(8, 128, 0, 0), (24, 256, 8, 128), (512, 4096, 16, 128)])
def test_flash_sizes_are_the_literal_formulas(R, Bp, R2, Bk):
    z = flash_sizes(R, Bp, R2, Bk)
    assert z.plane == Bp * 168
    assert z.pm == R * Bp and z.pl == R * Bp
    assert z.pO == R * Bp * 160
    assert z.pO2 == R2 * Bk * 160
    assert z.row == Bp
    assert z.part == Bp * 152
