"""Self-checks of oracle/bf16_step_ref.py, the row-wise float64 reference behind tests/test_gpu_bf16_rowwise.py (CPU only).
The closed forms on the bf16 operands must equal autograd of the same forward with straight-through operands; the float32 emulation of
the kernels' stated arithmetic must pass its own check on every input family and form of the GPU tests (upstream tensors from
x3_step_ref.synth_upstream), on inputs that hold enough rows only the gradient GEMM writes; and every planted fault must be rejected with
its quantity -- or table -- and its row named.

What the tensor-wide measures of tests/test_gpu_parity.py make of the same faults (asserted below, fault by fault):
  "6e-3" = every gradient tensor within 6e-3 of its maximum (test_bf16_logits_path_matches_bf16_aware_oracle, test_kd_fast_step_...);
  "share" = 99.9 % of theta within 2e-6, none beyond 1.1e-3, fewer than 1e-3 of the shadow elements different (test_fused_table_adam_
            equals_unfused_step, test_both_bf16_update_forms_agree).
    fault                                                     rejected here as                        tensor-wide measure
    one dense-only row of g scaled by 1 + 2^-7                g_dense, the row (rows sharing a direction) passes 6e-3
    one batch row missing from one tile                       g_dense                                 passes 6e-3
    target term from the float32 rep instead of rep_bf        g_sparse, a label row (label_rows)      passes 6e-3
    distilled rows not zeroed for items >= Np                 g_dense, a row > Np                     FAILS 6e-3 as well
    teacher term subtracted after the bf16 pack               g_dense (kd_near_ex1)                   passes 6e-3
    the two peeled head elements left un-updated              g_dense, row 65 (zero state); m         passes share
    the 2-float tail vector dropped                           g, row 128 (zero state); m              passes share
    a straddling shadow pair written into the wrong row       shadow, row 66 column 150               passes share
    one shadow row left stale                                 shadow, row 70                          passes share
    the EXTRA rows added to rows > N                          untouched rows: theta, row 651          invisible from zero state
    row N + 1 of a tail tile updated                          untouched rows: theta, row 651          passes share
    p not rounded to bf16 in the forward                      -- (one-sided measure, below)           passes 6e-3
All but one pass the measure that pins the bf16 step today.

The measure is ONE-SIDED (error <= bound): a forward that keeps p in float32 is CLOSER to the float64 reference and passes, as it
should -- it is not a wrong result.  What pins the stated rounding is the other direction: it is the emulated error of dRep, and a bound
computed from an emulation WITHOUT it is one that the stated arithmetic exceeds (test_the_rounding_of_p_is_the_error_of_drep).

What the measure can NOT see, asserted with its figures so that nobody reads more into a green run than it says.  The bound of a quantity
is 8 x the WORST row's emulated error, and in the bf16 step that error is the rounding of p: some 1e-3 of a GEMM row's term sum.
  * A 2^-7 scale of one dense-only row is two bf16 ulps on every term of the row.  On the independent synthetic rows of synth_upstream the
    terms of a row cancel as much as their roundings do: error 4.1e-3 against a bound of 1.16e-2 (N650).  It is rejected where the terms
    add up (300 rows that share a direction, as LayerNorm outputs do), and from 2^-5 on everywhere.
  * A label term taken from the float32 rep is half a bf16 ulp of that term.  Rows that only input positions touch are GEMM rows with a
    small exact term added and set the emulated error of g_sparse: 3.1e-3 against a bound of 6.4e-3 (N650).  In the label_rows family
    every row with sparse entries carries a label term and the fault is rejected; that family runs on the GPU for this reason.
  * The teacher term subtracted after the pack only ADDS roundings of the size the train rows' p have anyway when the exemplar rows weigh
    what the train rows weigh (70 + 70 rows: 1.2 x the emulated error).  It is rejected where one distilled row carries weight lambda
    beside 300 train rows and the teacher is close to the student: the kd_near_ex1 family, on the GPU for this reason."""
import functools

import numpy as np
import pytest
import torch

from oracle import ader_ref_cpu as R
from oracle import bf16_step_ref as Bf
from oracle import x3_step_ref as X

OUT = ("lse", "rowloss", "loss", "drep", "g")


@functools.lru_cache(maxsize=None)
def _built(name, form):
    """(case, batch, inputs, reference, emulation) of a family and form: computed once, shared, never modified."""
    case = Bf.BF16_CASE_BY_NAME[name]
    batch, inp = Bf.host_inputs(case)
    return case, batch, inp, Bf.reference_bf16(inp, form), Bf.emulate_bf16(inp, form)


def _as_dev(emu, **over):
    d = {k: emu[k].clone() if torch.is_tensor(emu[k]) else emu[k] for k in OUT}
    d.update(over)
    return d


def _rejects(dev, name, form, quantity, row=None):
    _, _, inp, ref, emu = _built(name, form)
    with pytest.raises(X.ParityError) as ei:
        Bf.check_bf16(dev, inp, form, ref=ref, emu=emu)
    msg = str(ei.value)
    assert quantity + ":" in msg, msg
    if row is not None:
        assert "worst rows %d " % row in msg, msg
    return msg


def _passes_6e3(g_fault, ref):
    """The tensor-wide measure of test_gpu_parity.py on the table gradient: within 6e-3 of its maximum."""
    return X.tensor_max_error(g_fault, ref["g"], X.NERR_FLOOR) < Bf.NERR_BF16


# ------------------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("name,form", [("N129", "sh"), ("onehot", "sh"), ("kd_Np64_ex70", "kd_fast"), ("kd_Np64_ex70", "kd_split")])
def test_closed_forms_equal_autograd_with_straight_through_operands(name, form):
    """reference_bf16 against float64 autograd of the same forward: the operands enter as x + (bf16(x) - x).detach(), so the values are
    the device's operands and the gradient flows to rep and the table unchanged.  Split distillation: the exemplar rows' logits come from
    the float32 operands."""
    case, batch, inp, _, _ = _built(name, form)
    N, n_train, B = inp["N"], inp["n_train"], inp["B"]
    w64 = torch.full((B,), 1.0 / n_train, dtype=torch.float64)
    w64[n_train:] = case["lam"] / max(B - n_train, 1)
    ref = Bf.reference_bf16(dict(inp, w=w64), form)
    rep = inp["rep"].double().requires_grad_(True)
    E = inp["E0"].double().requires_grad_(True)
    rep_st = rep + (inp["rep_bf"].double() - rep).detach()
    E_st = E + (inp["Esh"].double() - E).detach()
    logits = rep_st @ E_st[1:N + 1].t()
    if form == "kd_split":
        logits = torch.cat([logits[:n_train], rep[n_train:] @ E[1:N + 1].t()])
    loss = R.loss_tail(logits, batch["pos"], ex_logits=inp["tl"].double() if inp["tl"] is not None else None,
                       ex_pos=batch["ex_pos"], lambda_=case["lam"])
    real = inp["seq"] > 0
    lin = (inp["dx"].double()[real] * inp["sqrtH"] * E[inp["seq"][real]]).sum()
    (loss + lin).backward()
    rows = n_train if form == "kd_split" else B
    assert float((rep.grad[:rows] - ref["drep"]).abs().max()) <= 1e-12
    assert float((E.grad[1:N + 1] - ref["g"]).abs().max()) <= 1e-12
    assert float(E.grad[0].abs().max()) == 0.0 and float(E.grad[N + 1:].abs().max()) == 0.0
    with torch.no_grad():
        if form == "kd_split":          # the reference's loss is the train rows' share
            lsm = torch.log_softmax(logits[:n_train], -1)
            want = (-lsm[torch.arange(n_train), torch.as_tensor(batch["pos"]).long() - 1] * w64[:n_train]).sum()
        else:
            want = loss
        assert abs(float(want) - float(ref["loss"])) <= 1e-12 * max(1.0, abs(float(want)))
        for b in (0, n_train - 1, rows - 1):
            cols = inp["Np"] if (inp["tl"] is not None and b >= n_train) else N
            assert abs(float(torch.logsumexp(logits[b, :cols], -1)) - float(ref["lse"][b])) <= 1e-12
        assert float((ref["rowloss"].sum() - ref["loss"]).abs()) <= 1e-12


# ------------------------------------------------------------------------------------------- every input family and form
@pytest.mark.parametrize("name,form", Bf.BF16_RUNS, ids=["%s-%s" % r for r in Bf.BF16_RUNS])
def test_emulation_passes_and_inputs_hold_dense_only_rows(name, form):
    case, batch, inp, ref, emu = _built(name, form)
    assert X.dense_only_condition(inp) is None, X.dense_only_condition(inp)
    res = Bf.check_bf16(_as_dev(emu), inp, form, ref=ref, emu=emu)
    assert set(res) == set(X.QUANTITIES)
    for q, (err, base, bound) in res.items():
        assert err == base and bound >= X.FLOOR
    # float32 grade wherever no bf16 rounding enters: the log-sum-exp, and the one-hot rows' losses
    assert res["lse"][1] < 2.0 ** -20
    if form != "kd_fast":
        assert res["rowloss"][1] < 2.0 ** -20
    # p in bf16: half an ulp (2^-9) per term, never of order one.  (Not so dRep of a distilled row whose teacher is close to the student:
    # w (O / L - O2) is then the small difference of two readouts that were each rounded on their own -- some 2^-5 of ITS term sum.)
    assert res["g_dense"][1] < 2.0 ** -7 and res["g_sparse"][1] < 2.0 ** -7 and res["drep"][1] < (2.0 ** -4 if case.get("near") else 2.0 ** -8)
    if form == "sh":                    # the resident kernel's summation order is the same computation at this measure
        Bf.check_bf16(_as_dev(Bf.emulate_bf16(inp, "resident")), inp, "sh", ref=ref, emu=emu)


def test_cases_cover_the_forms_and_the_item_ranges():
    forms = {f for _, f in Bf.BF16_RUNS}
    assert forms == set(Bf.FORMS)
    assert sum(1 for _, f in Bf.BF16_RUNS if f == "kd_split") == 2
    # ader_lbf_ranges: 24 ranges of one block at N = 650 (three of them empty), 8 ranges with seven empty at N = 2 .. 32
    assert Bf.lbf_ranges(650, 128) == 24 and Bf.lbf_ranges(2, 128) == 8 and Bf.lbf_ranges(650, 384) == 24
    assert Bf.lbf_ranges_kd(650, 256, 128) == 24 and Bf.lbf_readout_ranges(650, 256, 128) == 24
    assert Bf.lbf_ranges(10 ** 6, 1024) == 64 and Bf.lbf_readout_ranges(10 ** 6, 256, 128) == 176
    # H % 4 == 2: every tile of the table starts 8 bytes past a 16-byte boundary; H % 4 == 0: none does
    for H, mis in ((150, True), (158, True), (10, True), (64, False), (160, False)):
        assert all(Bf.tile_is_misaligned(t, H) == mis for t in range(11))


# ------------------------------------------------------------------------------------------- planted faults: gradient
def _coherent_inputs():
    """lists_records' batch (B = 300) with representations that share a direction: rep = 0.3 randn + a common row."""
    case = Bf.BF16_CASE_BY_NAME["lists_records"]
    batch = X.make_batch(case)
    E0, rep, dx = X.synth_upstream(case, batch)
    g = torch.Generator().manual_seed(3)
    rep = 0.3 * torch.randn(rep.shape, generator=g) + (torch.randn(1, rep.shape[1], generator=g) * 1.1)
    return Bf.with_operands(X.inputs_of(case, batch, E0, rep, dx))


def test_a_scaled_dense_row_is_rejected_where_its_terms_add_up():
    """One dense-only row of g scaled by 1 + 2^-7 (two bf16 ulps on every term of the row)."""
    inp = _coherent_inputs()
    assert X.dense_only_condition(inp) is None
    ref, emu = Bf.reference_bf16(inp), Bf.emulate_bf16(inp)
    Bf.check_bf16(_as_dev(emu), inp, ref=ref, emu=emu)
    j = int(torch.nonzero(X.dense_only_rows(inp))[37])
    g = emu["g"].clone()
    g[j] *= 1 + 2.0 ** -7
    with pytest.raises(X.ParityError) as ei:
        Bf.check_bf16(_as_dev(emu, g=g), inp, ref=ref, emu=emu)
    assert "g_dense:" in str(ei.value) and "worst rows %d " % (j + 1) in str(ei.value), str(ei.value)
    assert _passes_6e3(g, ref)
    # ... on the independent rows of synth_upstream the same fault is inside the bound: the terms cancel as their roundings do
    _, _, inp2, ref2, emu2 = _built("N650", "sh")
    j2 = int(torch.nonzero(X.dense_only_rows(inp2))[37])
    g2 = emu2["g"].clone()
    g2[j2] *= 1 + 2.0 ** -7
    err, base, bound = Bf.check_bf16(_as_dev(emu2, g=g2), inp2, ref=ref2, emu=emu2)["g_dense"]
    print("\nN650: a 2^-7 scale of dense-only row %d: error %.3g, emulated %.3g, bound %.3g" % (j2 + 1, err, base, bound))
    assert 0.1 * bound < err < bound
    g2[j2] = emu2["g"][j2] * (1 + 2.0 ** -5)
    assert _rejects(_as_dev(emu2, g=g2), "N650", "sh", "g_dense", j2 + 1) and _passes_6e3(g2, ref2)


def test_check_rejects_a_batch_row_missing_from_one_tile():
    _, _, inp, ref, emu = _built("N650", "sh")
    g = emu["g"].clone()
    b = 41
    g[64:128] -= emu["c"][b, 64:128, None] * emu["rep_q"][b][None, :]
    _rejects(_as_dev(emu, g=g), "N650", "sh", "g_dense")
    assert _passes_6e3(g, ref)


def test_check_rejects_a_target_term_from_the_float32_rep():
    """In the label_rows family, where every row with sparse entries carries a label term.  In the other families the rows that only
    input positions touch set the emulated error of g_sparse (they are GEMM rows with a small exact term added), and half a bf16 ulp of
    the label term stays inside 8 x that: asserted with its figures on N650."""
    _, _, inp, ref, emu = _built("label_rows", "sh")
    bad = Bf.emulate_bf16(inp, "sh", fault="target_f32_rep")
    msg = _rejects(_as_dev(bad), "label_rows", "sh", "g_sparse")
    labels = set(int(v) for v in inp["y"].tolist())
    worst = int(msg.split("g_sparse:")[1].split("worst rows ")[1].split(" ")[0])
    assert worst in labels, msg
    assert "g_dense:" not in msg and _passes_6e3(bad["g"], ref)
    _, _, inp2, ref2, emu2 = _built("N650", "sh")
    bad2 = Bf.emulate_bf16(inp2, "sh", fault="target_f32_rep")
    err, base, bound = Bf.check_bf16(_as_dev(bad2), inp2, ref=ref2, emu=emu2)["g_sparse"]
    print("\nN650: label term from the float32 rep: g_sparse error %.3g, emulated %.3g, bound %.3g" % (err, base, bound))
    assert base < err < bound


@pytest.mark.parametrize("name", ["kd_Np645_ex70", "kd_Np64_ex70"])
def test_check_rejects_distilled_rows_not_zeroed_beyond_Np(name):
    _, _, inp, ref, emu = _built(name, "kd_fast")
    bad = Bf.emulate_bf16(inp, "kd_fast", fault="no_zero_Np")
    msg = _rejects(_as_dev(bad), name, "kd_fast", "g_dense")
    worst = int(msg.split("g_dense:")[1].split("worst rows ")[1].split(" ")[0])
    assert worst > inp["Np"], msg
    # (the one planted fault the tensor-wide measure sees as well: 70 whole terms in rows that hold nothing else of their size)
    assert torch.equal(bad["g"][:inp["Np"]], emu["g"][:inp["Np"]]) and not _passes_6e3(bad["g"], ref)


def _near_teacher_inputs(B, n_ex):
    """A distilled batch (Np = 648) with a teacher CLOSE to the student (Bf.set_near_teacher; B = 300, one exemplar row: the kd_near_ex1
    family of the GPU test)."""
    case = dict(X._case("kd_near", B=B, mode="kd", Np=648, n_ex=n_ex, lam=0.7), near=True)
    return Bf.host_inputs(case)[1]


def test_check_rejects_a_teacher_term_subtracted_after_the_bf16_pack():
    """Rejected where the exemplar row carries weight against the train rows' own roundings: one exemplar row (weight lambda) beside
    300 train rows (weight 1/300 each).  With 70 exemplar rows of the train rows' weight the fault only ADDS roundings of the size the
    70 train rows have anyway: asserted with its figures -- a measure that judges a table row as a whole cannot tell them apart."""
    inp = _near_teacher_inputs(300, 1)
    ref, emu = Bf.reference_bf16(inp, "kd_fast"), Bf.emulate_bf16(inp, "kd_fast")
    Bf.check_bf16(_as_dev(emu), inp, "kd_fast", ref=ref, emu=emu)
    bad = Bf.emulate_bf16(inp, "kd_fast", fault="sub_after_pack")
    with pytest.raises(X.ParityError) as ei:
        Bf.check_bf16(_as_dev(bad), inp, "kd_fast", ref=ref, emu=emu)
    assert "g_dense:" in str(ei.value) and "worst rows" in str(ei.value), str(ei.value)
    assert _passes_6e3(bad["g"], ref)
    inp = _near_teacher_inputs(70, 70)
    ref, emu = Bf.reference_bf16(inp, "kd_fast"), Bf.emulate_bf16(inp, "kd_fast")
    err, base, bound = Bf.check_bf16(_as_dev(Bf.emulate_bf16(inp, "kd_fast", fault="sub_after_pack")), inp, "kd_fast", ref=ref,
                                     emu=emu)["g_dense"]
    print("\n70 + 70 rows: teacher term subtracted after the pack: g_dense error %.3g, emulated %.3g, bound %.3g" % (err, base, bound))
    assert base < err < 2 * base


def test_the_rounding_of_p_is_the_error_of_drep():
    """One-sided measure: a forward that keeps p in float32 passes (it is closer to the reference); an emulation without the stated
    rounding gives a bound that the stated arithmetic itself exceeds -- in dRep, and in nothing else (g has its own, stated, rounding)."""
    _, _, inp, ref, emu = _built("N650", "sh")
    exact_p = Bf.emulate_bf16(inp, "sh", fault="p_f32")
    res = Bf.check_bf16(_as_dev(exact_p), inp, "sh", ref=ref, emu=emu)
    assert res["drep"][0] < 0.05 * res["drep"][1]
    assert torch.equal(exact_p["g"], emu["g"]) and _passes_6e3(exact_p["g"], ref)
    with pytest.raises(X.ParityError) as ei:
        Bf.check_bf16(_as_dev(emu), inp, "sh", ref=ref, emu=exact_p)
    assert "drep:" in str(ei.value) and "g_" not in str(ei.value) and "lse:" not in str(ei.value), str(ei.value)


# ------------------------------------------------------------------------------------------- planted faults: update, shadow, rows
def _update_setup(name, preloaded, extra=False):
    case, _, inp, _, emu = _built(name, "sh")
    k = X.adam_consts(5e-4, np.float32(0.9), np.float32(0.999))
    g = torch.Generator().manual_seed(5)
    th0 = inp["E0"]
    m0, v0 = torch.zeros_like(th0), torch.zeros_like(th0)
    if preloaded:
        m0 = torch.randn(th0.shape, generator=g) * 1e-3
        v0 = torch.rand(th0.shape, generator=g) * 1e-6
        m0[::7, ::5] = 0.0
        v0[::7, ::5] = 0.0
    sh0 = Bf.expected_shadow(th0)
    return inp["N"], k, th0, m0, v0, sh0, emu["g"]


def _update_checks(N, k, th0, m0, v0, sh0, g, fault, preloaded, inp=None, ref=None, emu=None, extra=None):
    """Everything the GPU test asserts behind the update, on update_emulate's tables.  Returns (theta, shadow) after the step."""
    th1, m1, v1, sh1 = Bf.update_emulate(th0, m0, v0, sh0, g, N, k, fault=fault, extra=extra)
    X.check_untouched((th0, m0, v0, sh0), (th1, m1, v1, sh1), N)
    Bf.check_shadow_after(sh1, th1, sh0, N)
    if preloaded:
        X.check_adam_preloaded(th0, m0, v0, th1, m1, v1, g.double(), N, k)
    else:
        g_dev = X.check_adam_zero(th0, th1, m1, v1, N, k)
        assert float((g_dev - g.double()).abs().max()) <= 2.0 ** -23 * float(g.abs().max()) or fault is not None
        if inp is not None:
            Bf.check_bf16(_as_dev(emu, g=g_dev), inp, ref=ref, emu=emu)
    return th1, sh1


@pytest.mark.parametrize("preloaded", [False, True])
def test_update_checks_pass_the_stated_update(preloaded):
    _, _, inp, ref, emu = _built("N650", "sh")
    _update_checks(*_update_setup("N650", preloaded), None, preloaded, inp, ref, emu)


# (fault, preloaded state, the words the rejection must hold)
UPDATE_REJECTIONS = [
    ("head", False, ("g_dense:", "worst rows 65 ")),            # zero state: m' = 0 in the two elements reads as a gradient of 0
    ("head", True, ("m (preloaded)", "(row 64, col ")),         # (check_adam_* number the rows 1..N from 0: table row 65)
    ("tail2", False, ("worst rows 128 ",)),                     # (row 128 is an ordinary id: g_sparse or g_dense as the batch has it)
    ("tail2", True, ("m (preloaded)", "row 127, col 148")),
    ("shadow_straddle", False, ("shadow after the step", "row 66, column 150")),
    ("shadow_straddle", True, ("shadow after the step", "row 66, column 150")),
    ("shadow_stale", False, ("shadow after the step", "row 70,")),
    ("shadow_stale", True, ("shadow after the step", "row 70,")),
    ("extra_beyond_N", True, ("theta: row 651 is outside 1..650 and was written",)),
    ("row_N1", False, ("theta: row 651 is outside 1..650 and was written",)),
    ("row_N1", True, ("theta: row 651 is outside 1..650 and was written",)),
]


@pytest.mark.parametrize("fault,preloaded,words", UPDATE_REJECTIONS, ids=["%s-%s" % (f, "preloaded" if p else "zero")
                                                                          for f, p, _ in UPDATE_REJECTIONS])
def test_update_checks_reject(fault, preloaded, words):
    """Faults of the optimiser phase at tile 1 (rows 65..128) of N650 (H = 150: misaligned tiles), each against ALL checks of the GPU
    test in their order; the tensor-wide share rule of test_gpu_parity.py lets every one of them through."""
    _, _, inp, ref, emu = _built("N650", "sh")
    setup = _update_setup("N650", preloaded)
    extra = None
    if fault == "extra_beyond_N":
        extra = torch.zeros_like(setup[2])          # (zero beyond N, as Engine.loss_and_grad leaves the gradient buffer)
    with pytest.raises(X.ParityError) as ei:
        _update_checks(*setup, fault, preloaded, inp, ref, emu, extra=extra)
    for wd in words:
        assert wd in str(ei.value), str(ei.value)
    if not preloaded:       # (the share rule is about steps from the engines' own state; the preloaded state is this test's device)
        good = Bf.update_emulate(*setup[2:6], setup[6], setup[0], setup[1])
        bad = Bf.update_emulate(*setup[2:6], setup[6], setup[0], setup[1], fault=fault, extra=extra)
        assert Bf.share_rule_passes(bad[0], good[0], bad[3], good[3])


def test_extra_rows_beyond_N_are_invisible_from_zero_state():
    """Why engine B preloads m and v in ALL rows: with zero state and a zero gradient Adam's update is exactly zero, so an optimiser phase
    that runs over rows > N (the EXTRA rows are zero there) changes no bit of theta, m or v -- only the preloaded run can see it."""
    setup = _update_setup("N650", False)
    _update_checks(*setup, "extra_beyond_N", False, extra=torch.zeros_like(setup[2]))


def test_operand_checks_name_the_row():
    case, batch, inp, _, _ = _built("kd_Np645_ex70", "kd_fast")
    n, n_ex, H = inp["n_train"], inp["B"] - inp["n_train"], inp["H"]
    plane = Bf.expected_rep_bf(inp["rep"], n, n_ex, True)
    assert plane.shape == (256, Bf.LDR) and bool((plane[n:128] == 0).all()) and bool((plane[128 + n_ex:] == 0).all())
    assert torch.equal(Bf.check_rep_bf(plane, inp["rep"], n, n_ex, True), inp["rep_bf"])
    bad = plane.clone()
    bad[128 + 3, :H] = (inp["rep"][n + 3].view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)      # truncated, not RNE
    with pytest.raises(X.ParityError) as ei:
        Bf.check_rep_bf(bad, inp["rep"], n, n_ex, True)
    assert "rep_bf: row 131," in str(ei.value)
    bad = plane.clone()
    bad[n, 0] = 1.0                                                 # a padding row of the train block
    with pytest.raises(X.ParityError) as ei:
        Bf.check_rep_bf(bad, inp["rep"], n, n_ex, True)
    assert "rep_bf: row %d, column 0" % n in str(ei.value)
    sh = Bf.expected_shadow(inp["E0"])
    assert torch.equal(Bf.check_shadow(sh, inp["E0"]), inp["Esh"])
    sh[17, H] = 1.0                                                 # a padding column
    with pytest.raises(X.ParityError) as ei:
        Bf.check_shadow(sh, inp["E0"])
    assert "shadow: row 17, column %d" % H in str(ei.value)


# ------------------------------------------------------------------------------------------- range launches
@pytest.mark.parametrize("name,W", Bf.RANGE_RUNS)
def test_tile_ranges_partition_the_rows(name, W):
    case = Bf.BF16_CASE_BY_NAME[name]
    N = case["N"]
    tiles, rows = Bf.tile_ranges(N, W, case["item_num"])
    covered = torch.zeros(N + 2, dtype=torch.int64)
    for (tb, tc), (lo, hi) in zip(tiles, rows):
        assert tc >= 1 and (hi < lo or (lo == 128 * tb + 1 and hi == min(128 * (tb + tc), N)))
        if hi >= lo:
            covered[lo:hi + 1] += 1
    assert bool((covered[1:N + 1] == 1).all()) and int(covered[0]) == 0 and int(covered[N + 1]) == 0
    # a range launch that also writes the tile behind its range is caught by the untouched-rows check, the shadow included
    th0 = torch.zeros(case["item_num"] + 1, 4)
    sh0 = torch.zeros(case["item_num"] + 1, Bf.LDR, dtype=torch.bfloat16)
    lo, hi = rows[0]
    sh1 = sh0.clone()
    sh1[min(hi + 1, case["item_num"]), 2] = 1.0
    with pytest.raises(X.ParityError) as ei:
        X.check_range_untouched((th0, th0, th0, sh0), (th0, th0, th0, sh1), lo, hi, 0)
    assert "shadow: rank 0's launch" in str(ei.value)
