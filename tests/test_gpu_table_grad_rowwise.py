"""Row-wise float64 parity of the table gradient that is WRITTEN OUT to Engine.grad, and of the dense Adam step behind it: the route
of loss_and_grad on its own, compute_fisher, every EWC step, the autograd ops and the dense data-parallel exchange.

Two forms, one loss_and_grad call per case and form (no optimiser), isolated at engine level as tests/test_gpu_x3_rowwise.py does:
    f32   logits_dtype = "f32": ader_logits_loss_fwd, ader_logits_bwd_drep, ader_logits_bwd_demb (logits.hip)
    x3u   logits_dtype = "x3":  ader_lx3_fwd_img_lnf + ader_tab_grad, a distilled step ader_lx3_fwd_kd_lnf + ader_tab_grad_kd
          (k_tab_upd<X3, ADAM = false> and k_tab_target_fix, table_update.hip)
both followed by ader_embed_bwd_rows and ader_scatter_rows_ordered (Engine._scatter_dx).  The device's OWN upstream is read back right
behind the synchronisation (rep, the masked and dropout-scaled per-position gradient rows, the table) and only the kernels downstream
of it are restated in float64 (oracle/x3_step_ref.py: reference; emulate_f32 / emulate(unfused=True) for the bound).  Every quantity
is judged ROW BY ROW in the term-sum measure against max(8 x the emulated float32 error on the same inputs, 16 float32 ulps), the
table rows that only the gradient GEMM writes apart from the rows with sparse entries.  Every run asserts which launchers ran and
which did not; a distilled x3 case that leaves the flash path fails.  Exact: gradient row 0 and the rows beyond max_item are bitwise
zero; after a second call with a smaller catalog (`shrink`) the rows it left behind are zero; for one row at rate 0 the Fisher
diagonal of compute_fisher is the square of that call's gradient.

Dense Adam (ader_adam_step over the whole flat buffer, Engine.adam): train_step with fuse_adam off, from zero state and from preloaded
m / v, table and every other parameter held elementwise to the float32 rounding bounds of check_adam_zero / check_adam_preloaded with
the device's own gradient; table rows 0 and > max_item stay bitwise untouched.

Shapes (oracle/x3_step_ref.GRAD_CASES): the 64-row chunks, the padding to 64 and MAXB = 1024 of the exact-f32 kernels, catalogs whose
item ranges hold no sub-tile (N <= 129) and one with 16 ranges (N = 1100), the x3 row counts of tests/test_gpu_x3_rowwise.py, labels
shared inside one workgroup of k_tab_target_fix and across three 64-row ballot blocks, shared labels with different weights.

Measured on an MI355X (device error / emulated error, worst over the cases; profiles/table_grad_rowwise_parity.txt has every line):
    f32   lse 2.36x   rowloss 2.49x   g_dense 1.81x   g_sparse 1.79x (all H10, each under the 16-ulp floor of 9.5e-07)
          drep 1.21x (B1)   loss 3.86x (lists_records: 8.8e-08, a 300-term float32 sum in another order; under the floor)
    x3u   lse 1.28x (kd_Np648_ex70)   rowloss 1.18x (N129)   drep 1.19x (H10)   g_dense 1.39x (shrink/2)   g_sparse 1.03x (kd_Np650_ex70)
          loss 5.69x (B1153: 5.6e-08, under the floor)
The bound is 8x: the unchanged kernels sit on the emulation in all 63 judged calls, every exact check holds and the 12 dense Adam runs
hold their rounding bounds.  The first run found the EMULATION short of a stated step: mma_tile carries one accumulator per output
through the k steps, and k_logits_bwd_de keeps it across the batch chunks -- a fmaf chain over all batch rows.  Emulated as blocked
float32 sums, the rows only the GEMM writes stood at 10.1x at B = 1024 (2.0e-06 of the term sum against 2.0e-07); emulated as the
chain (oracle/x3_step_ref._chain_mm) the ratio is 0.88x, and no kernel was changed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _engine  # noqa: E402

from oracle import x3_step_ref as X  # noqa: E402

LR = 5e-4
STEP0 = 3
RATE = 0.3
RUNS = [(c, f) for c in X.GRAD_CASES for f in c["forms"]]
RUN_IDS = ["%s-%s" % (c["name"], f) for c, f in RUNS]


def _host(t):
    return t.detach().clone().cpu()


def _make_engine(case, form, packed=False):
    eng = _engine(case["item_num"], case["T"], case["H"], 1, 1, seed=8, logits_dtype="f32" if form == "f32" else "x3")
    eng.pack_sessions = packed                  # (not packed: per-position gradient rows in position order)
    assert eng.lx3 == (form == "x3u") and eng.lfast == (form == "x3u") and eng.gemm_x3 == (case["H"] <= 150)
    eng.global_step = STEP0
    return eng


def _record_launches(monkeypatch):
    """Every launcher the engine calls from here on, by name (the engine modules bind `call` at import)."""
    import ader_amd.engine.backward as BW
    import ader_amd.engine.common as CM
    import ader_amd.engine.forward as FW
    import ader_amd.engine.update as UP
    launched = []
    orig = BW.call

    def call(name, *a):
        launched.append(name)
        return orig(name, *a)
    for mod in (BW, CM, FW, UP):
        assert mod.call is orig
        monkeypatch.setattr(mod, "call", call)
    return launched


def _step_kw(case, batch):
    if case["mode"] == "onehot":
        return dict(ex_pos=batch["ex_pos"], lambda_=case["lam"])
    if case["mode"] == "kd":
        return dict(teacher=torch.from_numpy(batch["teacher"]).cuda(), ex_trow=batch["trow"], lambda_=case["lam"])
    return {}


def check_launches(launched, form, mode):
    """The test is about THESE kernels: the launchers a form must have run, and the ones it must not."""
    ran = set(launched)
    if form == "f32":
        must = {"ader_logits_loss_fwd", "ader_logits_bwd_drep", "ader_logits_bwd_demb", "ader_scatter_rows_ordered"}
        never = {n for n in ran if n.startswith("ader_tab_grad") or n.startswith("ader_lx3_fwd")}
    elif mode == "kd":                           # (a distilled case off the flash path would run the exact-f32 kernels instead)
        must = {"ader_lx3_fwd_kd_lnf", "ader_tab_grad_kd", "ader_scatter_rows_ordered"}
        never = {n for n in ran if n.startswith("ader_logits_") and n not in ("ader_logits_ranges", "ader_logits_parts")} | (
            ran & {"ader_tab_grad", "ader_lx3_fwd_img_lnf"})
    else:
        must = {"ader_lx3_fwd_img_lnf", "ader_tab_grad", "ader_scatter_rows_ordered"}
        never = {n for n in ran if n.startswith("ader_logits_") and n not in ("ader_logits_ranges", "ader_logits_parts")} | (
            ran & {"ader_tab_grad_kd", "ader_lx3_fwd_kd_lnf"})
    never |= {n for n in ran if n.startswith("ader_tab_update")}        # no fused update of any kind (x3, sh, kd, ranged)
    assert must <= ran and not never, (sorted(must - ran), sorted(never))


def _loss_and_grad(eng, case, batch, form, launched):
    """One loss_and_grad (no optimiser); everything the checks need, cloned right behind the synchronisation."""
    H, N, B, n_ex = case["H"], case["N"], case["B"], case["n_ex"]
    Ba = B + n_ex
    E0 = _host(eng.param("emb"))
    del launched[:]
    loss = eng.loss_and_grad(batch["seq"], batch["pos"], N, rate=RATE, **_step_kw(case, batch))
    torch.cuda.synchronize()
    kd_flash = form == "x3u" and case["mode"] == "kd"
    ws = eng._ws
    out = dict(E0=E0, rep=_host(eng._act["rep"]), dx=_host(eng._last_g), lse=_host(ws["lg_lse"]), rowloss=_host(ws["lg_rowloss"]),
               drep=_host(ws["drep"]), loss=float(loss.item()), g_full=_host(eng.gradient("emb")),
               wrow=_host(ws["kf_w" if kd_flash else "ri_w"]))
    eng.check_status()
    check_launches(launched, form, case["mode"])
    assert eng._step.deferred is None and eng.global_step == STEP0                  # nothing deferred, no optimiser step
    assert torch.equal(_host(eng.param("emb")), E0)
    assert out["rep"].shape == (Ba, H) and out["drep"].shape == (Ba, H) and out["dx"].shape == (Ba * case["T"], H)
    rows, total = X.step_rows(B, n_ex, kd_flash, pad=64 if form == "f32" else 128)
    pad = torch.ones(total, dtype=torch.bool)
    pad[rows] = False
    for name in ("lse", "rowloss"):
        assert out[name].numel() == total and not bool(out[name][pad].any()), name      # padding rows: exact zeros
    assert torch.equal(out["wrow"][rows], X.step_weights(B, n_ex, case["lam"]))
    out["lse"], out["rowloss"] = out["lse"][rows], out["rowloss"][rows]
    return out


def _judge(label, form, case, batch, out):
    """check() of one call's outputs against the reference on the device's own upstream; prints the record line first."""
    N = case["N"]
    inp = X.inputs_of(case, batch, out["E0"], out["rep"], out["dx"])
    assert X.dense_only_condition(inp) is None
    ref = X.reference(inp)
    emu = X.emulate_f32(inp) if form == "f32" else X.emulate(inp, unfused=True)
    dev = dict(lse=out["lse"], rowloss=out["rowloss"], loss=out["loss"], drep=out["drep"], g=out["g_full"][1:N + 1])
    dense = X.dense_only_rows(inp)
    e_dev, e_emu = X.quantity_errors(dev, ref, dense), X.quantity_errors(emu, ref, dense)
    print("\ntable-grad %-18s %-3s %s" % (label, form, "  ".join(
        "%s %.2fx (%.2e)" % (q, float(e_dev[q].max()) / max(float(e_emu[q].max()), 1e-300), float(e_dev[q].max()))
        for q in X.QUANTITIES)))
    res = X.check(dev, inp, ref=ref, emu=emu)
    assert set(res) == set(X.QUANTITIES)
    last = out["g_full"].shape[0] - 1
    X.check_rows_zero(out["g_full"], 0, 0)
    if last > N:
        X.check_rows_zero(out["g_full"], N + 1, last)


@pytest.mark.parametrize("case,form", RUNS, ids=RUN_IDS)
def test_written_table_gradient_matches_rowwise_float64_reference(case, form, monkeypatch):
    batch = X.make_batch(case)
    eng = _make_engine(case, form)
    launched = _record_launches(monkeypatch)
    out = _loss_and_grad(eng, case, batch, form, launched)
    _judge(case["name"], form, case, batch, out)
    if case["then_N"]:
        # ---- the same engine, a smaller catalog: rows 1..N judged as in any case, the rows left behind exactly zero
        case2 = X.second_call(case)
        batch2 = X.make_batch(case2, 1)
        assert eng._grad_hi == case["N"] > case2["N"] and bool(out["g_full"][case2["N"] + 1:case["N"] + 1].any())
        out2 = _loss_and_grad(eng, case2, batch2, form, launched)
        _judge(case2["name"], form, case2, batch2, out2)
        X.check_rows_zero(out2["g_full"], case2["N"] + 1, case["N"], "gradient after the catalog shrank")
    if case["name"] == "B1":
        # ---- compute_fisher: one sample, dropout off; F = 0 + 1.0 * g * g is ONE rounded product of that call's gradient
        del launched[:]
        F = eng.compute_fisher(batch["seq"], batch["pos"], case["N"])
        torch.cuda.synchronize()
        eng.check_status()
        check_launches(launched, form, case["mode"])
        assert "ader_sq_accum" in launched and eng.global_step == STEP0
        g = _host(eng.grad)
        assert bool(g.any()) and torch.equal(_host(F), g * g)


@pytest.mark.parametrize("form", ["f32", "x3u"])
def test_packed_sessions_feed_the_same_scatter(form, monkeypatch):
    """The base family on packed session tiles: the input rows reach the scatter through dx_emb."""
    case = X.GRAD_CASE_BY_NAME["N650"]
    batch = X.make_batch(case)
    eng = _make_engine(case, form, packed=True)
    launched = _record_launches(monkeypatch)
    out = _loss_and_grad(eng, case, batch, form, launched)
    assert eng._act.get("pack") is not None and eng._last_g is eng._ws["dx_emb"]
    assert {"ader_seqp_fwd", "ader_seqp_bwd_qkv", "ader_pos_grad_packed"} <= set(launched)
    _judge(case["name"] + "/packed", form, case, batch, out)


def _column(t):
    """A flat parameter span as a one-column table with a row 0, the shape the Adam checks take."""
    return torch.cat([torch.zeros(1, dtype=t.dtype), t]).reshape(-1, 1)


@pytest.mark.parametrize("preload", [False, True], ids=["zero", "preloaded"])
@pytest.mark.parametrize("form", ["f32", "x3u"])
@pytest.mark.parametrize("name", X.ADAM_FAMILIES)
def test_dense_adam_step_holds_its_rounding_bounds(name, form, preload, monkeypatch):
    case = X.GRAD_CASE_BY_NAME[name]
    batch = X.make_batch(case)
    N, H = case["N"], case["H"]
    eng = _make_engine(case, form)
    eng.fuse_adam = False
    off, shp = eng.layout["emb"]
    span, tab_n = eng.layout["pos"][0], shp[0] * H
    # the table heads the flat buffer; behind its item_num + 1 rows lie the rows allocated for whole 128-item tiles, then the rest
    assert off == 0 and tuple(shp) == (case["item_num"] + 1, H) and tab_n <= span == min(o for o, _ in eng.layout.values() if o > 0)
    if preload:
        gen = torch.Generator().manual_seed(21)
        m0 = torch.zeros(eng.P)
        v0 = torch.zeros(eng.P)
        m0[H:(N + 1) * H] = torch.randn(N * H, generator=gen) * 1e-3           # table rows 1..N only
        v0[H:(N + 1) * H] = torch.rand(N * H, generator=gen) * 1e-6
        m0[span:] = torch.randn(eng.P - span, generator=gen) * 1e-3
        v0[span:] = torch.rand(eng.P - span, generator=gen) * 1e-6
        m0[::5] = 0.0                                                            # some exact zeros, in every kind of row
        v0[::5] = 0.0
        eng.adam_m.copy_(m0)
        eng.adam_v.copy_(v0)
    before = tuple(_host(t) for t in (eng.theta, eng.adam_m, eng.adam_v))
    k = X.adam_consts(LR, eng.b1p, eng.b2p, eng.beta1, eng.beta2, eng.eps)
    launched = _record_launches(monkeypatch)
    eng.train_step(batch["seq"], batch["pos"], N, LR, rate=RATE)
    torch.cuda.synchronize()
    eng.check_status()
    check_launches(launched, form, case["mode"])
    assert "ader_adam_step" in launched and eng._step.deferred is None and eng.global_step == STEP0 + 1
    after = tuple(_host(t) for t in (eng.theta, eng.adam_m, eng.adam_v))
    g_flat = _host(eng.grad)                                    # the device's own gradient, read after the step
    tab = lambda t: t[:tab_n].view(*shp)                        # noqa: E731
    for b, a in zip(before, after):                             # the allocated rows behind the table: zero gradient, never moved
        assert torch.equal(b[tab_n:span].view(torch.int32), a[tab_n:span].view(torch.int32))
    assert not bool(g_flat[tab_n:span].any())
    parts = [("table", tuple(tab(t) for t in before), tuple(tab(t) for t in after), tab(g_flat)[1:N + 1], N),
             ("other parameters", tuple(_column(t[span:]) for t in before), tuple(_column(t[span:]) for t in after),
              g_flat[span:].reshape(-1, 1), eng.P - span)]
    for what, b, a, g, n in parts:
        try:
            if preload:
                X.check_adam_preloaded(b[0], b[1], b[2], a[0], a[1], a[2], g, n, k)
            else:
                g_dev = X.check_adam_zero(b[0], a[0], a[1], a[2], n, k)
                # m' = g (1 - beta1) is one rounding: the gradient Adam consumed is the gradient in Engine.grad
                assert bool(((g_dev - g.double()).abs() <= 2.0 ** -23 * g.double().abs() + 2.0 ** -126).all()), what
        except X.ParityError as e:
            raise X.ParityError("%s: %s" % (what, e))
    X.check_untouched(parts[0][1], parts[0][2], N)              # table rows 0 and > N: zero gradient, zero state, not moved
