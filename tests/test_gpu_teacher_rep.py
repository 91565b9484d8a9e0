"""Distillation from stored teacher representations (engine.TeacherRep, ader_teacher_rows, --teacher_form rep).  The contract is
equality of bytes with the dense-teacher form at every level: the regenerated rows are the rows ader_logits_store wrote, a distilled
step fed a TeacherRep leaves the loss, theta and Adam state of the step fed the [E, Np] logits, and two periods of the driver log the
same metrics.  No tolerance anywhere: both sides run the same arithmetic."""
import functools
import itertools
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ITEM, T, H, L, N, NP = 700, 20, 150, 2, 650, 603          # Np odd: the 16-byte row stride of the materialised rows matters


def _engine(item_num=ITEM, T_=T, H_=H, L_=L, heads=1, seed=3, **kw):
    from ader_amd.engine import Engine
    kw.setdefault("logits_dtype", "x3")
    eng = Engine(item_num, maxlen=T_, hidden_units=H_, num_blocks=L_, num_heads=heads, seed=seed, **kw)
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


def _seqs(rs, B, T_, n_items):
    seq = np.zeros((B, T_), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, T_ + 1))
        seq[b, T_ - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _rows(trep, temb, ex_trow, n_ex, Np, E=None, fill=float("nan"), lse=False):
    """ader_teacher_rows through the C ABI into a buffer prefilled with `fill`: (rows [Bk, ldr], trow_local [Bk], lse [Bk] or None)."""
    from ader_amd._lib import call, ptr
    Bk, ldr = (n_ex + 63) // 64 * 64, (Np + 3) // 4 * 4
    dev = trep.device
    rows = torch.full((Bk, ldr), fill, device=dev)
    trl = torch.full((Bk,), -7, dtype=torch.int32, device=dev)
    z = torch.full((Bk,), fill, device=dev) if lse else None
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    call("ader_teacher_rows", ptr(trep), ptr(temb), ptr(ex_trow), n_ex, Bk, trep.shape[0] if E is None else E, trep.shape[1], Np,
         ptr(rows), ldr, ptr(trl), ptr(z), ptr(status), torch.cuda.current_stream().cuda_stream)
    assert int(status.item()) == 0
    return rows, trl, z


def _store(rep, temb, Np):
    """ader_logits_store of the rows of rep against items 1..Np of temb: [B, Np] (a view with a 16-byte row stride)."""
    from ader_amd._lib import call, ptr
    B, Hh = rep.shape
    Bp, ldo = (B + 63) // 64 * 64, (Np + 3) // 4 * 4
    ncol = torch.zeros(Bp, dtype=torch.int32, device=rep.device)
    ncol[:B] = Np
    out = torch.empty((B, ldo), device=rep.device)
    call("ader_logits_store", ptr(rep), ptr(temb), B, Bp, Hh, Np, ptr(ncol), ptr(out), ldo, torch.cuda.current_stream().cuda_stream)
    return out[:, :Np]


def _trow_variants(rs, n_ex, E):
    perm = rs.permutation(E)[:n_ex].astype(np.int32)
    dup = rs.randint(0, E, size=n_ex).astype(np.int32)
    if n_ex > 2:
        dup[1] = dup[0]
    holes = perm.copy()
    holes[[0, n_ex // 2, n_ex - 1]] = -1                  # padding rows at the start, in the middle and at the end
    return perm, dup, holes


# ------------------------------------------------------------------------------------------------------------- 1. rows, bit for bit
@pytest.mark.parametrize("Hh", [12, 64, 150])
def test_rows_are_the_bits_of_the_stored_logits(Hh):
    from ader_amd._lib import call
    rs = np.random.RandomState(100 + Hh)
    g = torch.Generator().manual_seed(Hh)
    for Np, n_ex, mult in itertools.product((1, 33, 63, 64, 65, 650, 4097), (1, 64, 65, 130), (1, 3)):
        E = mult * n_ex
        trep = torch.randn(E, Hh, generator=g).cuda()
        # the snapshot may be longer than Np + 1 rows: what lies behind item Np is never read (NaN there would reach the tile's last items)
        temb = torch.cat([torch.randn(Np + 1, Hh, generator=g) * 0.3, torch.full((3, Hh), float("nan"))]).cuda()
        Bk = (n_ex + 63) // 64 * 64
        if Np == 4097:
            assert (Np + 63) // 64 > call("ader_teacher_ranges", Np, Bk)            # a workgroup walks several tiles
        if Np == 650:
            assert (Np + 63) // 64 <= 4 * call("ader_teacher_ranges", Np, Bk)
        for tr in _trow_variants(rs, n_ex, E):
            trd = torch.from_numpy(tr).cuda()
            rows, trl, _ = _rows(trep, temb, trd, n_ex, Np)
            real = torch.zeros(Bk, dtype=torch.bool, device="cuda")
            real[:n_ex] = trd >= 0
            want = torch.zeros((Bk, Np), device="cuda")
            want[:n_ex] = _store(trep[trd.clamp(min=0).long()].contiguous(), temb, Np)
            want[~real] = 0.0                                                        # padding rows: exactly +0.0
            assert _same_bits(rows[:, :Np], want), (Hh, Np, n_ex, E)
            e = torch.arange(Bk, dtype=torch.int32, device="cuda")
            assert torch.equal(trl, torch.where(real, e, torch.full_like(e, -1))), (Hh, Np, n_ex, E)


def test_lse_output_is_ader_row_lse_of_the_rows():
    from ader_amd._lib import call, ptr
    g = torch.Generator().manual_seed(2)
    n_ex, E, Np = 37, 50, NP
    trep, temb = torch.randn(E, H, generator=g).cuda(), (torch.randn(Np + 1, H, generator=g) * 0.3).cuda()
    tr = torch.from_numpy(np.random.RandomState(2).randint(0, E, size=n_ex).astype(np.int32)).cuda()
    tr[5] = -1
    rows, trl, z = _rows(trep, temb, tr, n_ex, Np, lse=True)
    want = torch.full_like(z, float("nan"))
    call("ader_row_lse", ptr(rows), rows.stride(0), Np, ptr(trl), trl.shape[0], ptr(want), torch.cuda.current_stream().cuda_stream)
    assert _same_bits(z, want) and float(z[5]) == 0.0 and float(z[63]) == 0.0 and torch.isfinite(z).all()
    # ... and of the dense teacher's row (the stride differs, the arithmetic does not)
    dense = _store(trep, temb, Np)
    alls = torch.arange(E, dtype=torch.int32, device="cuda")
    zd = torch.empty(E, device="cuda")
    call("ader_row_lse", ptr(dense), dense.stride(0), Np, ptr(alls), E, ptr(zd), torch.cuda.current_stream().cuda_stream)
    keep = [e for e in range(n_ex) if e != 5]
    assert _same_bits(z[keep], zd[tr[keep].long()])


# ------------------------------------------------------------------------------------------------------------- 2. small integers
@pytest.mark.parametrize("Hh,Np,n_ex,E", [(150, 650, 130, 390), (12, 65, 65, 65), (64, 4097, 3, 9)])
def test_small_integer_operands_give_the_exact_integer_product(Hh, Np, n_ex, E):
    """Entries in -3..3: every product and partial sum is an exact float32, so the rows are the int64 product of the gathered rows --
    the gather and the indexing judged against something that is no kernel of this project."""
    rs = np.random.RandomState(Np)
    trep_i = rs.randint(-3, 4, size=(E, Hh))
    temb_i = rs.randint(-3, 4, size=(Np + 1, Hh))
    for tr in _trow_variants(rs, n_ex, E):
        rows, _, _ = _rows(torch.from_numpy(trep_i).float().cuda(), torch.from_numpy(temb_i).float().cuda(), torch.from_numpy(tr).cuda(),
                           n_ex, Np)
        want = np.zeros((rows.shape[0], Np), dtype=np.int64)
        ok = tr >= 0
        want[:n_ex][ok] = trep_i[tr[ok]].astype(np.int64) @ temb_i[1:Np + 1].astype(np.int64).T
        got = rows[:, :Np].cpu().numpy()
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32))


# ------------------------------------------------------------------------------------------------------------- 3. independence
def test_rows_do_not_depend_on_their_batch_and_calls_repeat():
    g = torch.Generator().manual_seed(4)
    E, n_ex, Np = 200, 130, 650
    trep, temb = torch.randn(E, H, generator=g).cuda(), (torch.randn(Np + 1, H, generator=g) * 0.3).cuda()
    tr = torch.from_numpy(np.random.RandomState(4).permutation(E)[:n_ex].astype(np.int32)).cuda()
    a, ta, _ = _rows(trep, temb, tr, n_ex, Np)
    b, tb, _ = _rows(trep, temb, tr, n_ex, Np, fill=7.0)
    assert _same_bits(a[:, :Np], b[:, :Np]) and torch.equal(ta, tb)
    for e in (0, 63, 64, 129):
        one, _, _ = _rows(trep, temb, tr[e:e + 1].contiguous(), 1, Np)
        assert _same_bits(one[0, :Np], a[e, :Np]), e


# ------------------------------------------------------------------------------------------------------------- 4. frozen snapshot
@functools.lru_cache(maxsize=None)
def _teachers():
    """The exemplar sessions, the dense teacher and the TeacherRep of ONE engine state (never written to afterwards)."""
    rs = np.random.RandomState(31)
    ex_seq = _seqs(rs, 50, T, NP)
    eng = _engine()
    dense = eng.teacher_logits(ex_seq, NP)
    trep = eng.teacher_rep(ex_seq, NP)
    torch.cuda.synchronize()
    return ex_seq, dense, trep


def test_the_snapshot_is_frozen():
    import ader_amd.ops  # noqa: F401
    rs = np.random.RandomState(32)
    ex_seq = _seqs(rs, 50, T, NP)
    eng = _engine()
    dense = eng.teacher_logits(ex_seq, NP).clone()
    trep = eng.teacher_rep(ex_seq, NP)
    assert trep.table.data_ptr() != eng.param("emb").data_ptr() and tuple(trep.table.shape) == (NP + 1, H) and len(trep) == 50
    before = eng.param("emb")[:NP + 1].clone()
    for _ in range(3):
        seq, pos = _seqs(rs, 70 + 37, T, N), rs.randint(1, N + 1, size=70).astype(np.int32)
        eng.train_step(seq, pos, N, 1e-2, rate=0.3, teacher=trep, ex_trow=rs.randint(0, 50, size=37).astype(np.int32), lambda_=0.7)
    torch.cuda.synchronize()
    eng.check_status()
    assert not torch.equal(before, eng.param("emb")[:NP + 1]) and torch.equal(before, trep.table)      # theta moved, the copy did not
    rows, trl = torch.ops.ader.teacher_rows(trep.rep, trep.table, torch.arange(50, dtype=torch.int32, device="cuda"), NP)
    assert _same_bits(rows[:50], dense) and torch.equal(trl[:50].cpu(), torch.arange(50, dtype=torch.int32))
    assert _same_bits(trep.rows(np.arange(7, 19)), dense[7:19])


def test_reference_shaped_view_of_a_rep_store_computes_the_dense_rows():
    from ader_amd.exemplar import ExemplarStore
    ex_seq, dense, trep = _teachers()
    rows = np.concatenate([ex_seq, np.random.RandomState(36).randint(1, 9, size=(50, 1)).astype(np.int32)], 1)
    by_r, by_d = ExemplarStore(rows, trep, NP).by_label(), ExemplarStore(rows, dense, NP).by_label()
    assert sorted(by_r) == sorted(by_d) and sum(len(v) for v in by_r.values()) == 50
    for label in by_d:
        for (sess_r, row_r), (sess_d, row_d) in zip(by_r[label], by_d[label]):
            assert sess_r == sess_d and _same_bits(row_r, row_d)


# ------------------------------------------------------------------------------------------------------------- 5. steps, bitwise
def _state(e):
    return float(e.loss.item()), e.theta.clone(), e.adam_m.clone(), e.adam_v.clone()


def _assert_same_state(a, b, what):
    assert np.float32(a[0]).tobytes() == np.float32(b[0]).tobytes(), (what, a[0], b[0])
    for x, y, name in zip(a[1:], b[1:], ("theta", "adam_m", "adam_v")):
        assert torch.equal(_bits(x), _bits(y)), (what, name)


@pytest.mark.parametrize("mode", ["x3", "x3-pack", "x3-unfused", "x3-split", "f32", "bf16", "bf16-pack"])
def test_distilled_steps_equal_the_dense_teacher_steps(mode):
    ex_seq, dense, trep = _teachers()
    n_t, n_e = 70, 37
    rs0 = np.random.RandomState(33)
    batches = [(_seqs(rs0, n_t + n_e, T, N), rs0.randint(1, N + 1, size=n_t).astype(np.int32),
                rs0.randint(0, 50, size=n_e).astype(np.int32)) for _ in range(4)]          # (37 draws of 50 rows: duplicates)
    assert any(len(set(b[2].tolist())) < n_e for b in batches)
    engines = []
    for teacher in (dense, trep):
        e = _engine(logits_dtype=mode.split("-")[0])
        e.pack_sessions = mode.endswith("-pack")
        e.fuse_adam = mode != "x3-unfused"
        e.kd_fast = mode != "x3-split"
        engines.append((e, teacher))
    for s, (seq, pos, tr) in enumerate(batches):
        got = []
        for e, teacher in engines:
            e.train_step(seq, pos, N, 1e-3, rate=0.3, teacher=teacher, ex_trow=tr, lambda_=0.7)
            torch.cuda.synchronize()
            e.check_status()
            got.append(_state(e))
        _assert_same_state(got[0], got[1], (mode, s))
    assert engines[1][0]._tlse_key is None                 # the rep form never touched the dense form's per-tensor lse cache
    assert engines[0][0]._tlse_key is not None


def test_loss_and_grad_takes_a_teacher_rep():
    ex_seq, dense, trep = _teachers()
    rs = np.random.RandomState(34)
    seq, pos, tr = _seqs(rs, 70 + 37, T, N), rs.randint(1, N + 1, size=70).astype(np.int32), rs.randint(0, 50, size=37).astype(np.int32)
    out = []
    for teacher in (dense, trep):
        e = _engine()
        e.loss_and_grad(seq, pos, N, teacher=teacher, ex_trow=tr, lambda_=0.7, rate=0.3)
        torch.cuda.synchronize()
        out.append((float(e.loss.item()), e.grad.clone()))
    assert out[0][0] == out[1][0] and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


# ------------------------------------------------------------------------------------------------------------- 6. native driver
@functools.lru_cache(maxsize=None)
def _fed_inputs():
    from ader_amd.data import pack_rows
    rs = np.random.RandomState(4)
    n_rows, n_ex_rows = 300, 60
    sessions = [rs.randint(1, N + 1, size=int(k)).tolist() for k in np.clip(rs.geometric(0.25, size=n_rows) + 1, 2, 30)]
    ex_sessions = [rs.randint(1, NP + 1, size=int(k)).tolist() for k in np.clip(rs.geometric(0.25, size=n_ex_rows) + 1, 2, 30)]
    rows_t = torch.from_numpy(pack_rows(sessions, T)[0]).cuda()
    rows_e = torch.from_numpy(pack_rows(ex_sessions, T)[0]).cuda()
    perm_t = torch.from_numpy(rs.permutation(n_rows)).cuda()
    perm_e = torch.from_numpy(rs.permutation(n_ex_rows)).cuda()
    eng = _engine()
    ex_seq = rows_e[:, :T].contiguous()
    dense, trep = eng.teacher_logits(ex_seq, NP), eng.teacher_rep(ex_seq, NP)
    g = torch.Generator().manual_seed(8)
    from ader_amd.engine import TeacherRep
    other = TeacherRep(torch.randn(n_ex_rows, H, generator=g).cuda(), (torch.randn(NP + 1, H, generator=g) * 0.2).cuda(), NP)
    torch.cuda.synchronize()
    return rows_t, rows_e, perm_t, perm_e, dense, trep, other


def _fed_run(teachers, native, verify=False, steps=6):
    rows_t, rows_e, perm_t, perm_e = _fed_inputs()[:4]
    Bt, Be = 64, 16
    e = _engine()
    e.pack_sessions, e.pack_density, e.native_step, e.plan_verify = "auto", 0.1, native, verify
    o_t = o_e = 0
    losses = []
    for s in range(steps):
        n_t, n_e = (Bt, Bt - 2, Bt)[s % 3], Be - 3                              # n_e < Be: padding exemplar rows in every step
        e.train_step_fed((rows_t, perm_t, o_t, n_t, Bt, rows_e, perm_e, o_e % 32, n_e, Be), N, 1e-3, 0.3,
                         teacher=teachers[s % len(teachers)], lambda_=0.6)
        losses.append(e.loss.clone())
        o_t = (o_t + n_t) % 200
        o_e += n_e
    torch.cuda.synchronize()
    e.check_status()
    return e, [float(x.item()) for x in losses]


def test_device_fed_native_steps_equal_the_dense_form():
    _, _, _, _, dense, trep, _ = _fed_inputs()
    ed, ld = _fed_run([dense], native=True)
    er, lr = _fed_run([trep], native=True)
    assert er.plan_hits > 0 and not er.plan_errors, (er.plan_hits, er.plan_misses, er.plan_errors)
    assert ld == lr
    _assert_same_state(_state(ed), _state(er), "fed")
    names = [n for p in er._plans.values() if p for n in p.names if n]
    assert "ader_teacher_rows" in names                                        # the materialisation is part of the replayed plan
    ev, lv = _fed_run([trep], native=True, verify=True)
    assert ev.plan_verified > 0 and not ev.plan_errors, (ev.plan_verified, ev.plan_errors)
    assert lv == lr
    _assert_same_state(_state(ev), _state(er), "fed-verify")


def test_alternating_teacher_reps_follow_the_one_they_are_given():
    _, _, _, _, _, a, b = _fed_inputs()
    nat, l_nat = _fed_run([a, b], native=True, steps=9)                        # A, B, A, B, ... one shape per three steps
    ref, l_ref = _fed_run([a, b], native=False, steps=9)
    assert ref.plan_hits == 0 and nat.plan_hits > 0 and not nat.plan_errors, (nat.plan_hits, nat.plan_misses, nat.plan_errors)
    assert l_nat == l_ref
    _assert_same_state(_state(nat), _state(ref), "A/B/A")
    only_a, l_a = _fed_run([a], native=False, steps=9)
    assert l_a != l_ref                                                        # (B is a different teacher: the comparison can fail)


# ------------------------------------------------------------------------------------------------------------- 7. errors
def test_errors():
    import ader_amd.ops  # noqa: F401
    from ader_amd import _lib
    from ader_amd.engine import TeacherRep
    ex_seq, dense, trep = _teachers()
    rs = np.random.RandomState(35)
    seq, pos, tr = _seqs(rs, 70 + 37, T, N), rs.randint(1, N + 1, size=70).astype(np.int32), rs.randint(0, 50, size=37).astype(np.int32)
    # the catalog-sharded scheme reads teacher columns by item shard: no TeacherRep (raised before any collective is issued)
    e2 = _engine(dp_rank=0, dp_world=2)
    e2.dp_mode = "catalog"
    for step in (lambda: e2.train_step(seq, pos, N, 1e-3, teacher=trep, ex_trow=tr, lambda_=0.7),
                 lambda: e2.loss_and_grad(seq, pos, N, teacher=trep, ex_trow=tr, lambda_=0.7)):
        with pytest.raises(RuntimeError, match="catalog"):
            step()
    # the record checks its tensors
    with pytest.raises(RuntimeError):
        TeacherRep(trep.rep.double(), trep.table, NP)
    with pytest.raises(RuntimeError):
        TeacherRep(trep.rep, trep.table.half(), NP)
    with pytest.raises(RuntimeError):
        TeacherRep(trep.rep, trep.table.t().contiguous().t(), NP)               # a non-contiguous table
    with pytest.raises(RuntimeError):
        TeacherRep(trep.rep, trep.table, NP + 1)
    # the engine checks the record against itself: hidden size, catalog, exemplar row count
    e = _engine()
    with pytest.raises(RuntimeError):
        e.train_step(seq, pos, N, 1e-3, teacher=TeacherRep(trep.rep[:, :64].contiguous(), trep.table[:, :64].contiguous(), NP),
                     ex_trow=tr, lambda_=0.7)
    with pytest.raises(RuntimeError):
        e.train_step(seq, pos, NP - 1, 1e-3, teacher=trep, ex_trow=tr, lambda_=0.7)          # Np > max_item
    with pytest.raises(RuntimeError):
        e.train_step(seq, pos, N, 1e-3, teacher=trep, ex_trow=tr[:30], lambda_=0.7)
    with pytest.raises(RuntimeError):
        torch.ops.ader.teacher_rows(trep.rep, trep.table.t().contiguous().t(), torch.zeros(4, dtype=torch.int32, device="cuda"), NP)
    with pytest.raises(RuntimeError):
        torch.ops.ader.teacher_rows(trep.rep, trep.table, torch.zeros(4, dtype=torch.int64, device="cuda"), NP)
    # a teacher row >= E is never read: the row is written as padding and the status word says so
    with pytest.raises(RuntimeError, match="teacher row"):
        torch.ops.ader.teacher_rows(trep.rep, trep.table, torch.tensor([1, 50, 2], dtype=torch.int32, device="cuda"), NP)
    # the launcher refuses each stated violation with -2 and enqueues nothing
    fn = _lib.load().ader_teacher_rows
    p = _lib.ptr
    rows = torch.zeros(64, 608, device="cuda")
    trl, ex = torch.zeros(64, dtype=torch.int32, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    ok = dict(n_ex=37, Bk=64, H=H, Np=NP, ldr=608)
    for bad in (dict(H=161), dict(Bk=96), dict(Bk=32, n_ex=20), dict(n_ex=65), dict(Np=0), dict(ldr=600), dict(ldr=606), dict()):
        a = dict(ok, **bad)
        rc = fn(p(trep.rep), p(trep.table), p(ex), a["n_ex"], a["Bk"], 50, a["H"], a["Np"], p(rows), a["ldr"], p(trl), None, None, st)
        assert rc == (-2 if bad else 0), (bad, rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 8. driver
def test_two_periods_of_the_driver_log_the_same_in_both_forms(monkeypatch):
    from ader_amd import exemplar as X
    from ader_amd import main as M
    stores = {}

    def run(form):
        kept = stores.setdefault(form, [])

        class Gen(X.ExemplarGenerator):
            def _make_store(self, model, sel_rows):
                out = super()._make_store(model, sel_rows)
                kept.append(self.store)
                return out
        monkeypatch.setattr(M, "ExemplarGenerator", Gen)
        with tempfile.TemporaryDirectory() as d:
            args = M.build_parser().parse_args(["--dataset", "DIGINETICA", "--max_periods", "2", "--num_epochs", "1", "--results_root", d,
                                                "--teacher_form", form])
            lines = []
            out = M.run(args, log=lambda s="": lines.append(str(s)))
            text = open(os.path.join(d, "DIGINETICA-ADER", "Training_logs.txt")).read()
        text = text[text.index("Continue Learning"):]
        logged = [ln for ln in text.splitlines() if not ln.startswith("Total time")]
        return out, [ln for ln in lines if not ln.startswith("Total time")], logged

    out_l, lines_l, text_l = run("logits")
    out_r, lines_r, text_r = run("rep")
    assert any(ln.startswith("epoch:1, test") for ln in text_l) and any(ln.startswith("Total saved exemplar:") for ln in text_l)
    assert lines_l == lines_r and text_l == text_r
    assert out_l["periods"] == out_r["periods"] and out_l["average"] == out_r["average"]
    assert len(stores["logits"]) == len(stores["rep"]) == 2
    for sl, sr in zip(stores["logits"], stores["rep"]):
        assert sl.form == "logits" and sr.form == "rep" and np.array_equal(sl.rows, sr.rows)
        E, Np = len(sr), sr.max_item
        held = sum(t.numel() * t.element_size() if isinstance(t, torch.Tensor) else np.asarray(t).nbytes for t in sr.tensors())
        assert held == E * 150 * 4 + (Np + 1) * 150 * 4 + np.asarray(sr.rows).nbytes                   # no [E, Np] tensor anywhere
        assert all(tuple(t.shape) != (E, Np) for t in sr.tensors()) and tuple(sl.teacher.shape) == (E, Np)
