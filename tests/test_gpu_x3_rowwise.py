"""Row-wise float64 parity of the headline kernels: the x3 loss forward (k_lx3p / k_lx3r + the merge launch) and the fused table
update k_tab32x3 (gradient GEMM + sparse rows + TF-Adam), each isolated at engine level.

One fused train step runs on the default engine (logits_dtype = "x3"); the device's OWN upstream tensors are read back (rep, the
per-position gradient rows, the table before the step) and only the kernel downstream of them is restated, in float64 on the CPU
(oracle/x3_step_ref.py).  Outputs are compared ROW BY ROW in the term-sum measure of that module: a table row that only the gradient
GEMM writes (99.8 % of the table at the workload; the tests' ids are drawn so that 3 rows in 4 are such rows) is judged against its
own size and not against the tensor's maximum, which the label and input rows set 100 to 1000 times higher.  The bound of every
quantity is max(8 x the error of a float32 emulation of the kernels' arithmetic on the same inputs, 16 float32 ulps); Adam has
derived float32 rounding bounds, from zero state and from preloaded m / v, and rows 0 and > N must stay bitwise untouched.

Shapes: the smallest at which each mechanism of table_update_x3.hip engages (64-row tiles in pairs, 32-row chunks, rows padded to
128, the 8-entry inline list record, the heavy path beyond 32 entries, 256-entry list fetches), one family per mechanism.

Measured on an MI355X (device error / emulated error, worst over the cases; profiles/x3_rowwise_parity.txt has every case):
    lse 1.28x (kd_Np648_ex70)   rowloss 1.18x (N129)   drep 1.19x (H10)   g_dense 1.08x (B1153)   g_sparse 1.07x (N63)
    loss 5.69x (B1153: 5.6e-08, a 1153-term float32 sum in another order; under the 16-ulp floor of 9.5e-07)
The bound is 8x: the unchanged kernels sit on the emulation.  Adam and the untouched rows hold their bounds in all 28 cases."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import _engine  # noqa: E402

from oracle import x3_step_ref as X  # noqa: E402

LR = 5e-4
STEP0 = 3


def _host(t):
    return t.detach().clone().cpu()


def _run_step(case, batch, preload):
    """One fused train step; everything the checks need, cloned right behind the synchronisation (the workspaces are reused)."""
    H, N, B, n_ex = case["H"], case["N"], case["B"], case["n_ex"]
    eng = _engine(case["item_num"], case["T"], H, 1, 1, seed=8, logits_dtype="x3")
    eng.pack_sessions = False                  # per-position gradient rows in position order
    # H = 158: the per-op float32 block GEMMs (the x3 GEMMs stop at H = 150) under the unchanged x3 logits and update
    assert eng.lx3 and eng.lfast and eng.fuse_adam and eng.gemm_x3 == (H <= 150)
    eng.global_step = STEP0
    m_all, v_all = eng.view(eng.adam_m, "emb"), eng.view(eng.adam_v, "emb")
    if preload:
        g = torch.Generator().manual_seed(21)
        m0 = torch.randn(m_all.shape, generator=g) * 1e-3
        v0 = torch.rand(v_all.shape, generator=g) * 1e-6
        m0[::5, ::3] = 0.0                     # some exact zeros, in every kind of row
        v0[::5, ::3] = 0.0
        m_all.copy_(m0)
        v_all.copy_(v0)
    before = tuple(_host(t) for t in (eng.param("emb"), m_all, v_all))
    k = X.adam_consts(LR, eng.b1p, eng.b2p, eng.beta1, eng.beta2, eng.eps)
    kw = {}
    if case["mode"] == "onehot":
        kw = dict(ex_pos=batch["ex_pos"], lambda_=case["lam"])
    elif case["mode"] == "kd":
        teacher = torch.from_numpy(batch["teacher"]).cuda()
        kw = dict(teacher=teacher, ex_trow=batch["trow"], lambda_=case["lam"])
    loss = eng.train_step(batch["seq"], batch["pos"], N, LR, rate=0.3, **kw)
    torch.cuda.synchronize()
    out = dict(rep=_host(eng._act["rep"]), lse=_host(eng._ws["lg_lse"]), rowloss=_host(eng._ws["lg_rowloss"]),
               off=_host(eng._ws["lbf_off"]), drep=_host(eng._ws["drep"]), dx=_host(eng._last_g), loss=float(loss.item()),
               wrow=_host(eng._ws["kf_w" if case["mode"] == "kd" else "ri_w"]),
               after=tuple(_host(t) for t in (eng.param("emb"), m_all, v_all)), before=before, k=k)
    eng.check_status()
    assert eng._step.deferred is None and eng.global_step == STEP0 + 1          # the fused update ran
    Ba = B + n_ex
    assert out["rep"].shape == (Ba, H) and out["drep"].shape == (Ba, H) and out["dx"].shape == (Ba * case["T"], H)
    # ---- row numbering of the per-row buffers: plain, or [train rows padded to 128 | exemplar rows] in a distilled step
    if case["mode"] == "kd":
        assert eng._ws.get("lbf_pO2") is not None                               # all rows on the flash path, teacher readout ran
        # the readout kernel: k_lx3r takes 16-byte aligned teacher rows (Np % 4 == 0) of at least one 32-item block at H = 150;
        # anything else runs the readout form of k_lx3_fwd
        out["readout"] = "k_lx3r" if (teacher.stride(0) % 4 == 0 and teacher.data_ptr() % 16 == 0 and case["Np"] >= 32
                                      and H == 150) else "k_lx3_fwd"
        assert out["readout"] == ("k_lx3_fwd" if case["Np"] % 4 else "k_lx3r")
    rows, total = X.step_rows(B, n_ex, case["mode"] == "kd")
    assert out["lse"].numel() == total
    pad = torch.ones(out["lse"].numel(), dtype=torch.bool)
    pad[rows] = False
    for name in ("lse", "rowloss"):
        assert out[name].numel() == pad.numel() and not bool(out[name][pad].any()), name     # padding rows: exact zeros
    assert bool(torch.isneginf(out["off"][pad]).all()) and bool(torch.isfinite(out["off"][rows]).all())
    assert torch.equal(out["wrow"][rows], X.step_weights(B, n_ex, case["lam"]))
    out["lse"], out["rowloss"] = out["lse"][rows], out["rowloss"][rows]
    return out


@pytest.mark.parametrize("case", X.CASES, ids=X.CASE_IDS)
def test_x3_step_matches_rowwise_float64_reference(case):
    batch = X.make_batch(case)
    N = case["N"]
    # ---- engine A, zero Adam state: forward, gradient (dense-only rows and rows with sparse entries apart), Adam from zero
    A = _run_step(case, batch, preload=False)
    inp = X.inputs_of(case, batch, A["before"][0], A["rep"], A["dx"])
    assert X.dense_only_condition(inp) is None
    k = A["k"]
    g_dev = A["after"][1][1:N + 1].double() / k["omb1"]
    dev = dict(lse=A["lse"], rowloss=A["rowloss"], loss=A["loss"], drep=A["drep"], g=g_dev)
    ref, emu = X.reference(inp), X.emulate(inp)
    try:
        res = X.check(dev, inp, ref=ref, emu=emu)
    finally:
        dense = X.dense_only_rows(inp)
        e_dev, e_emu = X.quantity_errors(dev, ref, dense), X.quantity_errors(emu, ref, dense)
        print("\nx3-rowwise %-16s %s%s" % (case["name"], "  ".join(
            "%s %.2fx (%.2e)" % (q, float(e_dev[q].max()) / max(float(e_emu[q].max()), 1e-300), float(e_dev[q].max()))
            for q in X.QUANTITIES), ("  readout " + A["readout"]) if "readout" in A else ""))
    assert set(res) == set(X.QUANTITIES)
    assert torch.equal(X.check_adam_zero(A["before"][0], A["after"][0], A["after"][1], A["after"][2], N, k), g_dev)
    X.check_untouched(A["before"], A["after"], N)
    # ---- engine B, same seed / batch / step, m and v preloaded in ALL table rows
    Bq = _run_step(case, batch, preload=True)
    real = inp["seq"] > 0                                               # (padding positions have no gradient row)
    for name in ("rep", "lse", "rowloss", "drep", "dx", "loss"):        # the step is reproducible: the same gradient went in
        same = (A[name] == Bq[name]) if name == "loss" else torch.equal(A[name][real] if name == "dx" else A[name],
                                                                        Bq[name][real] if name == "dx" else Bq[name])
        assert same, "%s differs between two runs of the same step" % name
    assert Bq["k"] == k
    X.check_adam_preloaded(Bq["before"][0], Bq["before"][1], Bq["before"][2], Bq["after"][0], Bq["after"][1], Bq["after"][2],
                           g_dev, N, k)
    X.check_untouched(Bq["before"], Bq["after"], N)
