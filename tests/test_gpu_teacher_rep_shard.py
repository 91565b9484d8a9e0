"""Distilling from a TeacherRep on the catalog-sharded table (ader_teacher_rows_shard, TeacherRep.lse, Engine._train_step_catalog).
The contract is equality of bytes with the dense-teacher form at every level: a rank's window holds the columns ader_logits_store /
ader_teacher_rows wrote, the captured log-sum-exps are ader_row_lse of the dense rows, and a distilled catalog-sharded step handed the
record leaves the loss, theta, Adam state and small parameters of the step handed the [E, Np] logits.  No tolerance anywhere: both
sides run the same arithmetic.  The teacher always comes from an engine whose table differs from the live one (another seed), so a
read of the live table in place of the snapshot shows."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000          # torch.full(..., nan)
ST_BAD_TROW = 2
# (Np, item_begin, item_count, n_loc): first shard; 316 items with a 60-item last tile; scalar tail (266 = 4 * 66 + 2); 18 items; empty
WINDOWS = ((700, 0, 384, 384), (700, 384, 384, 316), (650, 384, 384, 266), (530, 512, 256, 18), (500, 512, 256, 0))
E_ST, N_LIST, BK = 70, 37, 64


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _listed_rows(rs):
    """37 listed rows of the 70 stored ones: repeats, and -1 at the start, in the middle and at the end."""
    tr = rs.randint(0, E_ST, size=N_LIST).astype(np.int32)
    tr[3] = tr[2]
    tr[[0, 17, N_LIST - 1]] = -1
    return tr


def _operands(Hh, Np):
    g = torch.Generator().manual_seed(1000 * Hh + Np)
    trep = torch.randn(E_ST, Hh, generator=g).cuda()
    # the snapshot is longer than Np + 1 rows: what lies behind item Np is never read (NaN there would reach a tile's last items)
    temb = torch.cat([torch.randn(Np + 1, Hh, generator=g) * 0.3, torch.full((3, Hh), float("nan"))]).cuda()
    return trep, temb


def _dense_rows(trep, temb, ex, n_ex, Np, E=None):
    """ader_teacher_rows: (rows [BK, Np padded to 4], trow_local, status)."""
    from ader_amd._lib import call, ptr
    ldr = (Np + 3) // 4 * 4
    rows = torch.full((BK, ldr), float("nan"), device="cuda")
    trl = torch.full((BK,), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("ader_teacher_rows", ptr(trep), ptr(temb), ptr(ex), n_ex, BK, trep.shape[0] if E is None else E, trep.shape[1], Np, ptr(rows), ldr,
         ptr(trl), None, ptr(status), _st())
    return rows, trl, int(status.item())


def _window(trep, temb, ex, n_ex, Np, ib, ic, ldr, E=None):
    """ader_teacher_rows_shard into NaN-filled memory with a guard row on either side: (buffer [BK + 2, ldr], trow_local, status)."""
    from ader_amd._lib import call, ptr
    buf = torch.full((BK + 2, ldr), float("nan"), device="cuda")
    trl = torch.full((BK,), -7, dtype=torch.int32, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call("ader_teacher_rows_shard", ptr(trep), ptr(temb), ptr(ex), n_ex, BK, trep.shape[0] if E is None else E, trep.shape[1], Np, ib, ic,
         ptr(buf[1:]), ldr, ptr(trl), ptr(status), _st())
    return buf, trl, int(status.item())


# ------------------------------------------------------------------------------------------------------------- 1. the launcher
@pytest.mark.parametrize("Hh", [150, 50])           # 50: a zero-padded last k-step
def test_window_is_the_dense_rows_columns_and_nothing_else_is_written(Hh):
    import ader_amd.ops  # noqa: F401
    from ader_amd._lib import call, ptr
    rs = np.random.RandomState(Hh)
    tr = _listed_rows(rs)
    ex = torch.from_numpy(tr).cuda()
    real = torch.zeros(BK, dtype=torch.bool, device="cuda")
    real[:N_LIST] = ex >= 0
    e = torch.arange(BK, dtype=torch.int32, device="cuda")
    want_trl = torch.where(real, e, torch.full_like(e, -1))
    for Np, ib, ic, n_loc in WINDOWS:
        trep, temb = _operands(Hh, Np)
        dense, dtrl, dst = _dense_rows(trep, temb, ex, N_LIST, Np)
        assert dst == 0 and torch.equal(dtrl, want_trl)
        # ... which are ader_logits_store's bits for the listed rows
        ncol = torch.zeros(BK, dtype=torch.int32, device="cuda")
        ncol[:N_LIST] = Np
        stored = torch.empty((N_LIST, dense.shape[1]), device="cuda")
        call("ader_logits_store", ptr(trep[ex.clamp(min=0).long()].contiguous()), ptr(temb), N_LIST, BK, Hh, Np, ptr(ncol), ptr(stored),
             stored.stride(0), _st())
        keep = real[:N_LIST]
        assert _same_bits(dense[:N_LIST, :Np][keep], stored[:, :Np][keep])
        ldr = 384
        buf, trl, status = _window(trep, temb, ex, N_LIST, Np, ib, ic, ldr)
        assert status == 0 and torch.equal(trl, want_trl), (Np, ib)
        win = buf[1:BK + 1]
        assert _same_bits(win[:, :n_loc], dense[:, ib:ib + n_loc]), (Hh, Np, ib)
        assert bool((win[~real][:, :n_loc] == 0).all()) and not bool(torch.signbit(win[~real][:, :n_loc]).any())      # padding: +0.0
        # every byte outside [0, n_loc) of each row keeps its NaN bits (the guard rows too); on the empty shard every byte does
        assert bool((_bits(win[:, n_loc:]) == NAN_BITS).all()) and bool((_bits(buf[0]) == NAN_BITS).all()), (Np, ib)
        assert bool((_bits(buf[BK + 1]) == NAN_BITS).all())
        if n_loc == 0:
            assert bool((_bits(buf) == NAN_BITS).all())
        # the tightest row stride the launcher takes
        ldr_t = (n_loc + 3) // 4 * 4
        if 0 < ldr_t < ldr:
            buf_t, trl_t, _ = _window(trep, temb, ex, N_LIST, Np, ib, ic, ldr_t)
            assert _same_bits(buf_t[1:BK + 1, :n_loc], dense[:, ib:ib + n_loc]) and torch.equal(trl_t, want_trl)
            assert bool((_bits(buf_t[1:BK + 1, n_loc:]) == NAN_BITS).all()) and bool((_bits(buf_t[[0, BK + 1]]) == NAN_BITS).all())
        # the operator and the launcher agree
        rows_op, trl_op = torch.ops.ader.teacher_rows_shard(trep, temb, ex, Np, ib, ic)
        assert tuple(rows_op.shape) == (BK, n_loc) and torch.equal(trl_op, want_trl)
        assert _same_bits(rows_op, win[:, :n_loc])
        # a teacher row >= E is never read: written as padding, flagged (here E is lowered, so rows 60..69 are "beyond")
        buf_e, trl_e, status_e = _window(trep, temb, ex, N_LIST, Np, ib, ic, ldr, E=60)
        over = torch.zeros(BK, dtype=torch.bool, device="cuda")
        over[:N_LIST] = ex >= 60
        assert bool(over.any()) and status_e & ST_BAD_TROW
        assert torch.equal(trl_e, torch.where(real & ~over, e, torch.full_like(e, -1)))
        want_e = dense[:, ib:ib + n_loc].clone()
        want_e[over] = 0.0
        assert _same_bits(buf_e[1:BK + 1, :n_loc], want_e)
    with pytest.raises(RuntimeError, match="teacher row"):
        torch.ops.ader.teacher_rows_shard(trep, temb, torch.tensor([1, E_ST, 2], dtype=torch.int32, device="cuda"), 500, 0, 256)


def test_launcher_refuses_what_it_states():
    from ader_amd import _lib
    trep, temb = _operands(150, 700)
    fn = _lib.load().ader_teacher_rows_shard
    p = _lib.ptr
    rows = torch.zeros(BK, 384, device="cuda")
    trl, ex = torch.zeros(BK, dtype=torch.int32, device="cuda"), torch.zeros(BK, dtype=torch.int32, device="cuda")
    ok = dict(n_ex=N_LIST, Bk=BK, H=150, Np=700, ib=384, ic=384, ldr=384)
    for bad in (dict(ib=386), dict(ib=-4), dict(ic=-1), dict(ldr=382), dict(ldr=312), dict(H=161), dict(Bk=96), dict(Bk=32, n_ex=20),
                dict(n_ex=65), dict(Np=0), dict()):
        a = dict(ok, **bad)
        rc = fn(p(trep), p(temb), p(ex), a["n_ex"], a["Bk"], E_ST, a["H"], a["Np"], a["ib"], a["ic"], p(rows), a["ldr"], p(trl), None,
                _st())
        assert rc == (-2 if bad else 0), (bad, rc)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- 2. capture
ITEM, T, H, L = 900, 50, 150, 2


def _engine(item_num=ITEM, seed=4, **kw):
    from ader_amd.engine import Engine
    kw.setdefault("logits_dtype", "x3")
    eng = Engine(item_num, maxlen=T, hidden_units=H, num_blocks=L, num_heads=1, seed=seed, **kw)
    g = torch.Generator().manual_seed(seed + 11)
    for k in eng.layout:
        if k.endswith("_b"):
            eng.param(k).copy_(torch.randn(eng.layout[k][1], generator=g) * 0.1)
    eng.refresh_shadow()
    return eng


def _seqs(rs, B, n_items):
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


def test_captured_lse_is_ader_row_lse_of_the_dense_teacher():
    from ader_amd._lib import call, ptr
    eng = _engine(seed=9)
    for Np in (700, 650):
        ex_seq = _seqs(np.random.RandomState(Np), E_ST, Np)
        dense = eng.teacher_logits(ex_seq, Np)
        want = torch.full((E_ST,), float("nan"), device="cuda")
        alls = torch.arange(E_ST, dtype=torch.int32, device="cuda")
        call("ader_row_lse", ptr(dense), dense.stride(0), Np, ptr(alls), E_ST, ptr(want), _st())
        trep = eng.teacher_rep(ex_seq, Np, lse=True, chunk_rows=64)                   # one full chunk and a ragged one of 6 rows
        assert trep.lse.dtype == torch.float32 and tuple(trep.lse.shape) == (E_ST,) and trep.lse.is_contiguous()
        assert bool(torch.isfinite(want).all()) and _same_bits(trep.lse, want), Np
        assert _same_bits(eng.teacher_rep(ex_seq, Np, lse=True).lse, want)             # the default chunk: all rows at once
        bare, bare2 = eng.teacher_rep(ex_seq, Np), eng.teacher_rep(ex_seq, Np, lse=False)
        assert bare.lse is None and bare2.lse is None and bare.Np == trep.Np == Np
        assert _same_bits(bare.rep, trep.rep) and _same_bits(bare.table, trep.table) and tuple(bare.table.shape) == (Np + 1, H)
    with pytest.raises(RuntimeError, match="chunk_rows"):
        eng.teacher_rep(ex_seq, 650, lse=True, chunk_rows=96)


# ------------------------------------------------------------------------------------------------------------- 3. steps
B, N_EX, E_T = 96, 24, 40
# (W, packed exchange, item_num, max_item, Np, the shard size the engine must arrive at)
CASES = {"w2-dense-700": (2, False, 900, 830, 700, 512), "w2-packed-650": (2, True, 900, 830, 650, 512),
         "w3-dense-500": (3, False, 760, 740, 500, 256),            # the third rank owns no item below Np
         "w3-dense-530": (3, False, 760, 740, 530, 256)}            # ... or 18 of them: the readout kernel that takes any shape


def _poison_allocator():
    """NaN bit patterns in the caching allocator's free blocks: workspace that a kernel reads but nobody wrote shows in the result."""
    blocks = [torch.full((n,), float("nan"), device="cuda") for n in (128, 4096, 65536, 1 << 20, 1 << 22, 1 << 24) for _ in range(6)]
    torch.cuda.synchronize()
    del blocks


def _step_data(N, Np):
    rs = np.random.RandomState(Np)
    steps = [(_seqs(rs, B, N), rs.randint(1, N + 1, size=B).astype(np.int32), _seqs(rs, N_EX, Np),
              rs.randint(0, E_T, size=N_EX).astype(np.int32)) for _ in range(3)]
    return _seqs(rs, E_T, Np), steps


def _run(rank, world, packed, item_num, N, S, teacher, steps):
    from ader_amd import dist as adist
    eng = _engine(item_num, dp_rank=rank, dp_world=world)
    assert eng.shard_items == S
    dp = adist.DataParallel(eng, rank, world)
    eng.dp_mode, eng.dp_pack = "catalog", packed
    _poison_allocator()
    lo, hi = adist.shard_bounds(B, world, rank)
    elo, ehi = adist.shard_bounds(N_EX, world, rank)
    losses = []
    for seq, pos, ex_seq, trow in steps:
        dp.set_rows(lo, N, ex_row0=B + elo)
        eng.train_step(np.concatenate([seq[lo:hi], ex_seq[elo:ehi]]), pos[lo:hi], N, 5e-4, rate=0.3, teacher=teacher,
                       ex_trow=trow[elo:ehi], lambda_=0.6, n_train_global=B, n_ex_global=N_EX)
        losses.append(eng.loss.clone())
    eng.sync_table()
    torch.cuda.synchronize()
    eng.check_status()
    own = slice(H * (1 + rank * S), H * (1 + (rank + 1) * S))
    span = eng.layout["pos"][0]
    return dict(loss=torch.stack(losses).view(-1), theta=eng.theta[:(item_num + 1) * H].clone(), m=eng.adam_m[own].clone(),
                v=eng.adam_v[own].clone(), small=eng.theta[span:].clone(), small_m=eng.adam_m[span:].clone(),
                small_v=eng.adam_v[span:].clone())


def _step_worker(rank, world, port, case):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _, packed, item_num, N, Np, S = CASES[case]
    ex_all, steps = _step_data(N, Np)
    teng = _engine(item_num, seed=21)                      # the teacher: ANOTHER table than the live one's
    dense = teng.teacher_logits(ex_all, Np)
    trep = teng.teacher_rep(ex_all, Np, lse=True)
    assert trep.lse is not None and not torch.equal(trep.table, _engine(item_num).param("emb")[:Np + 1])
    a = _run(rank, world, packed, item_num, N, S, dense, steps)
    b = _run(rank, world, packed, item_num, N, S, trep, steps)
    assert bool(torch.isfinite(a["loss"]).all()) and bool(torch.isfinite(a["theta"]).all())
    assert not torch.equal(a["theta"], _engine(item_num).theta[:(item_num + 1) * H])          # the steps moved the table
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (case, rank, k, a["loss"].tolist(), b["loss"].tolist())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", sorted(CASES))
def test_catalog_sharded_steps_from_a_teacher_rep_equal_the_dense_teacher_steps(case):
    """Three distilled catalog-sharded steps, dropout on, run twice by every rank from engines with equal seeds -- once handed the
    dense teacher, once the TeacherRep (with lse) of the same teacher engine -- leave the same bytes on that rank: the loss of every
    step, theta after sync_table, the Adam moments of its shard's rows, the small parameters and their moments."""
    world = CASES[case][0]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_step_worker, args=(world, port, case), nprocs=world, join=True)


# ------------------------------------------------------------------------------------------------------------- 4. refusal
def test_a_record_without_lse_is_refused_before_any_collective():
    eng = _engine(dp_rank=0, dp_world=2)                   # no process group exists: a collective would raise something else
    eng.dp_mode = "catalog"
    rs = np.random.RandomState(3)
    ex_seq = _seqs(rs, E_T, 700)
    trep = _engine(seed=21).teacher_rep(ex_seq, 700)
    seq, pos, tr = _seqs(rs, 70 + 37, 830), rs.randint(1, 831, size=70).astype(np.int32), rs.randint(0, E_T, size=37).astype(np.int32)
    for step in (lambda: eng.train_step(seq, pos, 830, 1e-3, teacher=trep, ex_trow=tr, lambda_=0.7),
                 lambda: eng.loss_and_grad(seq, pos, 830, teacher=trep, ex_trow=tr, lambda_=0.7)):
        with pytest.raises(RuntimeError, match="catalog.*lse=True"):
            step()
