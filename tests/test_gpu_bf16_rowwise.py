"""Row-wise float64 parity of the bf16 step: the flash loss forward (k_lbf_fwd + k_lbf_combine) and the fused table updates
k_tab16<false,false> ("sh", the default), k_tab16<false,true> ("kd_fast"), k_tab16<true,false> ("kd_split") and the theta-resident
k_tab_upd<false,true> ("resident"), each isolated at engine level as tests/test_gpu_x3_rowwise.py does for the x3 step.

One fused train step runs on an engine with logits_dtype = "bf16"; the device's OWN upstream tensors are read back (rep, the operand
plane rep_bf, the table and its bf16 shadow before the step, the per-position gradient rows) and only what is downstream of them is
restated (oracle/bf16_step_ref.py).  Operands exact: rep_bf and the shadow are checked BITWISE against bf16(rep) / bf16(theta), padding
zero, before the step, and the shadow again after it.  Arithmetic row-wise: every row of lse, rowloss, dRep and both row classes of the
table gradient within max(8 x the error of the float32 emulation of the kernels' stated arithmetic, 16 float32 ulps) of the float64
closed forms ON THOSE OPERANDS.  Adam holds the derived float32 bounds from zero state (engine A; the gradient is read from m / (1 - b1))
and from m / v preloaded in ALL rows (engine B, whose forward tensors must equal A's bit for bit); row 0, the rows > N and the shadow
rows beyond the table stay bitwise untouched in theta, m, v and the shadow.  Every run asserts which launchers ran.

Range launches (the replicated row-sharded update): the TableJob of a step is captured before it is issued and issued through
issue_table_job for the tile ranges of W = 2, 3 simulated ranks on copies of theta / m / v / shadow: each launch leaves the rows outside
its range bitwise untouched, and the W launches together equal the single full launch bit for bit.

Shapes: the smallest at which each mechanism of these kernels engages (bf16_step_ref.BF16_CASES): 64-row tiles, 32-item blocks in >= 8
item ranges of which some are empty, 64-row rep chunks, rows padded to 128, H % 4 == 2 (misaligned tiles: the peeled head, the 2-float
tail, bf16 pairs across row ends) and H % 4 == 0, the 3 prefetched / 8 inline list entries, the heavy path, 256-entry fetches, a catalog
that fills the table.  (H = 160 is not a width the engine takes: hidden_units <= 159.)

Measured on an MI355X (device error / emulated error, worst over the 50 runs; profiles/bf16_rowwise_parity.txt has every run):
    lse 1.31x (kd_Np648_ex70 kd_fast)   rowloss 1.40x (N128)   loss 1.63x (N2: 8.9e-09, under the 16-ulp floor)
    drep 1.00x   g_dense 1.00x   g_sparse 1.00x   in EVERY run (0.98x once): their error is the stated rounding of p to bf16
The bound is 8x: the unchanged kernels sit on the emulation.  Operands, shadow, Adam, untouched rows, launchers and range launches hold
in all runs; no kernel was found wrong."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _engine  # noqa: E402

from oracle import bf16_step_ref as Bf  # noqa: E402
from oracle import x3_step_ref as X  # noqa: E402

LR = 5e-4
STEP0 = 3
FWD = {"sh": "ader_lbf_fwd", "resident": "ader_lbf_fwd", "kd_fast": "ader_lbf_fwd_kd", "kd_split": "ader_lbf_fwd"}
UPD = {"sh": "ader_tab_update_sh", "resident": "ader_tab_update", "kd_fast": "ader_tab_update_sh_kd", "kd_split": "ader_tab_update_sh"}


def _host(t):
    return t.detach().clone().cpu()


def _make_engine(case, form):
    eng = _engine(case["item_num"], case["T"], case["H"], 1, 1, seed=8, logits_dtype="bf16")
    eng.pack_sessions = False                  # per-position gradient rows in position order
    assert eng.lfast and not eng.lx3 and eng.fuse_adam and eng.shadow is not None and eng.bf16_update == "sh"
    if form == "resident":
        eng.bf16_update = "resident"
    if form == "kd_split":
        eng.kd_fast = False
    eng.global_step = STEP0
    return eng


def _tables(eng):
    return (eng.param("emb"), eng.view(eng.adam_m, "emb"), eng.view(eng.adam_v, "emb"), eng.shadow.view(-1, Bf.LDR))


def _step_kw(case, batch):
    if case["mode"] == "onehot":
        return dict(ex_pos=batch["ex_pos"], lambda_=case["lam"])
    if case["mode"] == "kd":
        return dict(teacher=torch.from_numpy(batch["teacher"]).cuda(), ex_trow=batch["trow"], lambda_=case["lam"])
    return {}


def _record_launches(monkeypatch):
    """Wrap the launcher entry of the modules that issue the loss forward and the table update (as tests/test_gpu_seq_stage.py does)."""
    import ader_amd.engine.backward as BW
    import ader_amd.engine.common as CM
    launched = []
    orig = BW.call
    assert CM.call is orig

    def call(name, *a):
        launched.append((name, a))
        return orig(name, *a)
    monkeypatch.setattr(BW, "call", call)
    monkeypatch.setattr(CM, "call", call)
    return launched


def _run_step(case, batch, form, preload, monkeypatch):
    """One fused train step; everything the checks need, cloned right behind the synchronisation (the workspaces are reused)."""
    H, N, B, n_ex = case["H"], case["N"], case["B"], case["n_ex"]
    eng = _make_engine(case, form)
    m_all, v_all = eng.view(eng.adam_m, "emb"), eng.view(eng.adam_v, "emb")
    if preload:
        g = torch.Generator().manual_seed(21)
        m0 = torch.randn(m_all.shape, generator=g) * 1e-3
        v0 = torch.rand(v_all.shape, generator=g) * 1e-6
        m0[::5, ::3] = 0.0                     # some exact zeros, in every kind of row
        v0[::5, ::3] = 0.0
        m_all.copy_(m0)
        v_all.copy_(v0)
    before = tuple(_host(t) for t in _tables(eng))
    k = X.adam_consts(LR, eng.b1p, eng.b2p, eng.beta1, eng.beta2, eng.eps)
    launched = _record_launches(monkeypatch)
    loss = eng.train_step(batch["seq"], batch["pos"], N, LR, rate=0.3, **_step_kw(case, batch))
    torch.cuda.synchronize()
    monkeypatch.undo()
    eng.check_status()
    assert eng._step.deferred is None and eng.global_step == STEP0 + 1          # the fused update ran
    kd, split = form == "kd_fast", form == "kd_split"
    nb, ne = (B, 0) if split else ((B, n_ex) if kd else (B + n_ex, 0))          # rows of the flash path: train, distilled
    ws = eng._ws
    out = dict(rep=_host(eng._act["rep"]), rep_bf=_host(ws["lbf_rep"]), lse=_host(ws["lg_lse"]), rowloss=_host(ws["lg_rowloss"]),
               off=_host(ws["lbf_off"]), drep=_host(ws["drep"]), dx=_host(eng._last_g), loss=float(loss.item()),
               wrow=_host(ws["kf_w" if kd else "ri_w"]), after=tuple(_host(t) for t in _tables(eng)), before=before, k=k)
    if split:       # the loss scalar holds both halves: the exemplar rows' half (exact-f32 kernels) is taken off again, in float64
        out["loss"] = out["loss"] - float(ws["kd_loss"].item())
    # ---- which kernels ran
    names = [n for n, _ in launched]
    assert names.count(FWD[form]) == 1 and names.count(UPD[form]) == 1, names
    assert not any(n.startswith("ader_lx3") or n.startswith("ader_tab_update_x3") for n in names), names
    assert [n for n in names if n.startswith("ader_tab_update")] == [UPD[form]] and [n for n in names if n.startswith("ader_lbf_fwd")] == [FWD[form]]
    if form in ("sh", "kd_split", "resident"):          # EXTRA instantiation: the dense extra gradient is the second-to-last argument
        extra = dict(launched)[UPD[form]][-2]
        assert (extra is not None and extra != 0) == split
    assert ("ader_logits_bwd_demb" in names) == split
    Ba = B + n_ex
    assert out["rep"].shape == (Ba, H) and out["drep"].shape == (Ba, H) and out["dx"].shape == (Ba * case["T"], H)
    rows, total = X.step_rows(nb, ne, kd)
    assert out["lse"].numel() == total and out["rep_bf"].numel() == total * Bf.LDR
    pad = torch.ones(total, dtype=torch.bool)
    pad[rows] = False
    for name in ("lse", "rowloss"):
        assert not bool(out[name][pad].any()), name                                          # padding rows: exact zeros
    assert bool(torch.isneginf(out["off"][pad]).all()) and bool(torch.isfinite(out["off"][rows]).all())
    assert torch.equal(out["wrow"][rows], X.step_weights(B, n_ex, case["lam"])[:nb + ne])
    out["lse"], out["rowloss"], out["rows"] = out["lse"][rows], out["rowloss"][rows], (nb, ne, kd)
    return out


@pytest.mark.parametrize("name,form", Bf.BF16_RUNS, ids=["%s-%s" % r for r in Bf.BF16_RUNS])
def test_bf16_step_matches_rowwise_float64_reference(name, form, monkeypatch):
    case = Bf.BF16_CASE_BY_NAME[name]
    batch = Bf.make_batch(case)
    N, H = case["N"], case["H"]
    if case.get("near"):        # the representations do not depend on the teacher: a first run gives the student the teacher is near to
        P = _run_step(case, batch, form, False, monkeypatch)
        Bf.set_near_teacher(case, batch, P["rep"][case["B"]:], P["before"][0])
    # ---- engine A, zero Adam state
    A = _run_step(case, batch, form, False, monkeypatch)
    assert not case.get("near") or torch.equal(A["rep"], P["rep"])
    nb, ne, kd = A["rows"]
    # operands, bitwise: the shadow before the step, the operand plane of the rows on the flash path
    Esh = Bf.check_shadow(A["before"][3], A["before"][0], "shadow before the step")
    rep_bf = Bf.check_rep_bf(A["rep_bf"], A["rep"][:nb + ne], nb, ne, kd)
    if form == "kd_split":
        rep_bf = torch.cat([rep_bf, Bf.bf16r(A["rep"][nb:]).float()])       # (the exemplar rows have no operand plane: unused)
    inp = Bf.with_operands(X.inputs_of(case, batch, A["before"][0], A["rep"], A["dx"]), rep_bf, Esh)
    assert X.dense_only_condition(inp) is None
    k = A["k"]
    g_dev = A["after"][1][1:N + 1].double() / k["omb1"]
    dev = dict(lse=A["lse"], rowloss=A["rowloss"], loss=A["loss"], drep=A["drep"][:nb + ne], g=g_dev)
    ref, emu = Bf.reference_bf16(inp, form), Bf.emulate_bf16(inp, form)
    try:
        res = Bf.check_bf16(dev, inp, form, ref=ref, emu=emu)
    finally:
        dense = X.dense_only_rows(inp)
        e_dev, e_emu = X.quantity_errors(dev, ref, dense), X.quantity_errors(emu, ref, dense)
        print("\nbf16-rowwise %-16s %-8s %s" % (case["name"], form, "  ".join(
            "%s %.2fx (%.2e)" % (q, float(e_dev[q].max()) / max(float(e_emu[q].max()), 1e-300), float(e_dev[q].max()))
            for q in X.QUANTITIES)))
    assert set(res) == set(X.QUANTITIES)
    assert torch.equal(X.check_adam_zero(A["before"][0], A["after"][0], A["after"][1], A["after"][2], N, k), g_dev)
    X.check_untouched(A["before"], A["after"], N)
    Bf.check_shadow_after(A["after"][3], A["after"][0], A["before"][3], N)
    # ---- engine B, same seed / batch / step, m and v preloaded in ALL table rows
    Bq = _run_step(case, batch, form, True, monkeypatch)
    real = inp["seq"] > 0                                               # (padding positions have no gradient row)
    for nm in ("rep", "rep_bf", "lse", "rowloss", "off", "drep", "dx", "loss"):     # the step is reproducible: the same gradient went in
        same = (A[nm] == Bq[nm]) if nm == "loss" else torch.equal(A[nm][real] if nm == "dx" else A[nm],
                                                                  Bq[nm][real] if nm == "dx" else Bq[nm])
        assert same, "%s differs between two runs of the same step" % nm
    assert Bq["k"] == k
    X.check_adam_preloaded(Bq["before"][0], Bq["before"][1], Bq["before"][2], Bq["after"][0], Bq["after"][1], Bq["after"][2],
                           g_dev, N, k)
    X.check_untouched(Bq["before"], Bq["after"], N)
    Bf.check_shadow_after(Bq["after"][3], Bq["after"][0], Bq["before"][3], N)


@pytest.mark.parametrize("name,W", Bf.RANGE_RUNS, ids=["%s-W%d" % r for r in Bf.RANGE_RUNS])
def test_range_launches_write_their_rows_only_and_add_up_to_the_full_launch(name, W):
    from ader_amd.engine.common import issue_table_job
    case = Bf.BF16_CASE_BY_NAME[name]
    batch = Bf.make_batch(case)
    N, H = case["N"], case["H"]
    eng = _make_engine(case, "sh")
    captured = {}
    eng._table_update = lambda job, lists, lr_t, **kw: captured.update(job=job, lists=lists, lr_t=lr_t, kw=kw)      # not issued
    eng.train_step(batch["seq"], batch["pos"], N, LR, rate=0.3)
    torch.cuda.synchronize()
    eng.check_status()
    job, lists, lr_t = captured["job"], captured["lists"], captured["lr_t"]
    assert captured["kw"] == {"bf16": "sh"} and job.lo is None and job.teacher is None and job.extra is None and job.N == N
    th0, m0, v0, sh0 = (t.detach().clone() for t in _tables(eng))
    g = torch.Generator().manual_seed(22)
    m0.copy_(torch.randn(m0.shape, generator=g) * 1e-3)          # state in ALL rows: a touched row changes whatever its gradient is
    v0.copy_(torch.rand(v0.shape, generator=g) * 1e-6)
    Bf.check_shadow(sh0, th0)

    def launch(tabs, tile_begin, tile_count):
        issue_table_job(job, lists, tabs[:3], eng.item_num, H, tabs[3], None, lr_t, eng.beta1, eng.beta2, eng.eps, eng._stream(),
                        tile_begin, tile_count, "sh")
        torch.cuda.synchronize()
    full = tuple(t.clone() for t in (th0, m0, v0, sh0))
    launch(full, 0, -1)
    X.check_untouched((th0, m0, v0, sh0), full, N)
    Bf.check_shadow_after(full[3], full[0], sh0, N)
    assert not torch.equal(full[0][1:N + 1], th0[1:N + 1])
    tiles, rows = Bf.tile_ranges(N, W, eng.item_num)
    cur = tuple(t.clone() for t in (th0, m0, v0, sh0))
    for r, ((tb, tc), (lo, hi)) in enumerate(zip(tiles, rows)):
        prev = tuple(t.clone() for t in cur)
        launch(cur, tb, tc)
        X.check_range_untouched(prev, cur, lo, hi, r)
        if hi >= lo:        # ... and the rows inside are the full launch's
            for nm, a, b in zip(X.TABLES, cur, full):
                assert torch.equal(a[lo:hi + 1], b[lo:hi + 1]), "%s: rank %d's rows differ from the full launch" % (nm, r)
    for nm, a, b in zip(X.TABLES, cur, full):
        assert torch.equal(a, b), "%s: the %d range launches together differ from the full launch" % (nm, W)
