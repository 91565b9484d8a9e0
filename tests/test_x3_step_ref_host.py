"""Self-checks of oracle/x3_step_ref.py, the row-wise float64 reference behind tests/test_gpu_x3_rowwise.py (CPU only).
The closed forms must equal autograd; the float32 emulation of the kernels' arithmetic must pass its own check on every input
family of the GPU tests, and those inputs must hold enough rows that only the gradient GEMM writes; check() must reject each of
eight planted faults (as test_plain_oracle_check_catches_a_wrong_mask does for the model oracle)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ader_ref_cpu as R
from oracle import x3_step_ref as X

CASE = {c["name"]: c for c in X.CASES}


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, batch, inputs, reference, emulation) of a family: computed once, shared, never modified."""
    case = CASE[name]
    batch = X.make_batch(case)
    inp = X.inputs_of(case, batch, *X.synth_upstream(case, batch))
    return case, batch, inp, X.reference(inp), X.emulate(inp)


def _as_dev(emu, **over):
    d = {k: emu[k].clone() if torch.is_tensor(emu[k]) else emu[k] for k in ("lse", "rowloss", "loss", "drep", "g")}
    d.update(over)
    return d


def _rejects(dev, name, quantity):
    _, _, inp, ref, emu = _built(name)
    with pytest.raises(X.ParityError) as ei:
        X.check(dev, inp, ref=ref, emu=emu)
    assert quantity in str(ei.value), str(ei.value)


# ------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("name", ["N129", "onehot", "kd_Np130_ex70"])
def test_closed_forms_equal_autograd(name):
    """lse, row losses, loss, dRep and the table gradient of reference() against float64 autograd through the loss tail of the model
    oracle (vanilla, one-hot exemplars, distillation with Np < N), the sparse term as the linear functional sqrt(H) sum dx . E[id]."""
    case, batch, inp, _, _ = _built(name)
    N, n_train = inp["N"], inp["n_train"]
    # (the kernels receive the row weights as C floats; the model oracle divides in float64: compare at ITS weights)
    w64 = torch.full((inp["B"],), 1.0 / n_train, dtype=torch.float64)
    w64[n_train:] = case["lam"] / max(inp["B"] - n_train, 1)
    assert float((w64 - inp["w"].double()).abs().max()) <= 2.0 ** -24 * float(w64.max())
    ref = X.reference(dict(inp, w=w64))
    rep = inp["rep"].double().requires_grad_(True)
    E = inp["E0"].double().requires_grad_(True)
    logits = rep @ E[1:N + 1].t()
    lam = case["lam"]
    loss = R.loss_tail(logits, batch["pos"], ex_logits=inp["tl"].double() if inp["tl"] is not None else None,
                       ex_pos=batch["ex_pos"], lambda_=lam)
    real = inp["seq"] > 0
    lin = (inp["dx"].double()[real] * inp["sqrtH"] * E[inp["seq"][real]]).sum()
    (loss + lin).backward()
    assert case["mode"] != "kd" or inp["Np"] < N
    assert abs(float(loss.detach()) - float(ref["loss"])) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    assert float((rep.grad - ref["drep"]).abs().max()) <= 1e-12
    assert float((E.grad[1:N + 1] - ref["g"]).abs().max()) <= 1e-12
    assert float(E.grad[0].abs().max()) == 0.0 and float(E.grad[N + 1:].abs().max()) == 0.0
    # per row: lse over the row's own columns, and the row's share of the loss
    with torch.no_grad():
        for b in (0, n_train - 1, inp["B"] - 1):
            cols = inp["Np"] if (inp["tl"] is not None and b >= n_train) else N
            assert abs(float(torch.logsumexp(logits[b, :cols], -1)) - float(ref["lse"][b])) <= 1e-12
        lsm = torch.log_softmax(logits[:n_train], -1)
        ce = -lsm[torch.arange(n_train), torch.as_tensor(batch["pos"]).long() - 1] * w64[:n_train]
        assert float((ce - ref["rowloss"][:n_train]).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------- every input family
@pytest.mark.parametrize("name", X.CASE_IDS)
def test_emulation_passes_and_inputs_hold_dense_only_rows(name):
    case, batch, inp, ref, emu = _built(name)
    assert X.dense_only_condition(inp) is None, X.dense_only_condition(inp)
    ordinary = set(int(i) for i in np.arange(4, case["N"] + 1, 4)) | {case["N"]}
    planted = {5, 70, 133, 197, 261, 262, 330, 645, 650, 77, 400, 401, 200} if case["plant"] else set()
    used = set(int(i) for i in inp["seq"].tolist()) | set(int(i) for i in inp["y"].tolist())
    assert used - {0} <= ordinary | planted
    res = X.check(_as_dev(emu), inp, ref=ref, emu=emu)
    for q, (err, base, bound) in res.items():
        assert err == base and bound >= X.FLOOR
        assert base < 2.0 ** -13, (q, base)             # float32 grade: a handful of 2^-16 products, nothing of order one
    # accumulating the gradient GEMM in the device's 32-row chunks is the same computation at this measure
    X.check(_as_dev(X.emulate(inp, chunk=32)), inp, ref=ref, emu=emu)


def test_list_families_hold_the_planted_list_lengths():
    """The list lengths the planted cases are about, per 64-id tile: 8 / 9 (inline record), 32 / 33 (heavy threshold), a bucket beyond
    256 entries whose second id's run straddles entry 256, a bucket heavy in the label list only, hot ids in the tail tile and in
    both tiles of a pair."""
    def per_tile(ids):
        ids = ids[ids > 0]
        return np.bincount((ids - 1) // X.TI, minlength=11)
    _, batch, _, _, _ = _built("lists_records")
    sp = per_tile(batch["seq"].reshape(-1))
    assert list(sp[:6]) == [8, 9, 32, 33, 43, 40] and sp[10] == 52
    assert per_tile(batch["pos"])[:6].sum() == 0
    _, batch, _, _, _ = _built("lists_hot")
    s = np.sort(batch["seq"].reshape(-1))
    s = s[s > 0]
    assert (s == 77).sum() == 600 and (batch["pos"] == 77).sum() == 120
    t6 = s[(s - 1) // X.TI == 6]
    assert len(t6) == 270 and t6[249] == 400 and t6[250] == 401 and t6[255] == 401 and t6[256] == 401
    assert per_tile(batch["seq"].reshape(-1))[3] == 0 and per_tile(batch["pos"])[3] == 40


# ------------------------------------------------------------------------------------------- planted faults
def test_check_rejects_a_scaled_dense_term():
    _, _, inp, _, emu = _built("N650")
    j = int(torch.nonzero(X.dense_only_rows(inp))[37])
    g = emu["g"].clone()
    g[j] *= 1 + 2.0 ** -10
    _rejects(_as_dev(emu, g=g), "N650", "g_dense")


def test_check_rejects_a_batch_row_missing_from_one_tile():
    _, _, inp, _, emu = _built("N650")
    g = emu["g"].clone()
    b = 41
    g[64:128] -= emu["c"][b, 64:128, None] * emu["rep_q"][b][None, :]
    _rejects(_as_dev(emu, g=g), "N650", "g_dense")


def test_check_rejects_a_dropped_entry_of_a_hot_row():
    _, _, inp, _, emu = _built("lists_hot")
    k = int(torch.nonzero(inp["seq"] == 77)[300])
    g = emu["g"].clone()
    g[76] -= inp["dx"][k] * np.float32(inp["sqrtH"])
    _rejects(_as_dev(emu, g=g), "lists_hot", "g_sparse")


def test_check_rejects_an_exemplar_label_term_with_the_train_weight():
    _, _, inp, _, emu = _built("onehot")
    b = inp["n_train"] + 3
    w = inp["w"]
    assert float(w[b]) != float(w[0])
    g = emu["g"].clone()
    g[int(inp["y"][b]) - 1] += (w[b] - w[0]) * emu["rep_q"][b]
    _rejects(_as_dev(emu, g=g), "onehot", "g_sparse")


def test_check_rejects_a_student_softmax_over_all_items():
    _, _, inp, _, _ = _built("kd_Np130_ex70")
    ncol = torch.full((inp["B"],), inp["N"], dtype=torch.int64)
    ncol[inp["n_train"]:] = inp["Np"]
    ncol[inp["n_train"] + 5] = inp["N"]                  # one distilled row normalised over N instead of Np
    _rejects(_as_dev(X.emulate(inp, ncol=ncol)), "kd_Np130_ex70", "lse")


def _adam_setup(preloaded):
    _, _, inp, _, emu = _built("N650")
    k = X.adam_consts(5e-4, np.float32(0.9), np.float32(0.999))
    g = torch.Generator().manual_seed(5)
    th0 = inp["E0"]
    m0, v0 = torch.zeros_like(th0), torch.zeros_like(th0)
    if preloaded:
        m0 = torch.randn(th0.shape, generator=g) * 1e-3
        v0 = torch.rand(th0.shape, generator=g) * 1e-6
        m0[::7, ::5] = 0.0
        v0[::7, ::5] = 0.0
    return inp["N"], k, th0, m0, v0, emu["g"]


def _adam_checks(N, k, th0, m0, v0, g, fault, preloaded):
    th1, m1, v1 = X.adam_emulate(th0, m0, v0, g, N, k, fault=fault)
    X.check_untouched((th0, m0, v0), (th1, m1, v1), N)
    if preloaded:
        X.check_adam_preloaded(th0, m0, v0, th1, m1, v1, g.double(), N, k)
    else:
        g_dev = X.check_adam_zero(th0, th1, m1, v1, N, k)
        assert float((g_dev - g.double()).abs().max()) <= 2.0 ** -23 * float(g.abs().max())


@pytest.mark.parametrize("preloaded", [False, True])
def test_adam_checks_pass_the_float32_formula(preloaded):
    _adam_checks(*_adam_setup(preloaded), None, preloaded)


@pytest.mark.parametrize("preloaded", [False, True])
@pytest.mark.parametrize("fault,word", [("eps_in_sqrt", "theta"), ("v_from_old_m", "v ("), ("row_N1", "was written")])
def test_adam_checks_reject(fault, word, preloaded):
    with pytest.raises(X.ParityError) as ei:
        _adam_checks(*_adam_setup(preloaded), fault, preloaded)
    assert word in str(ei.value), str(ei.value)
