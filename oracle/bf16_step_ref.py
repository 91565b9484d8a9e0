"""Row-wise float64 reference of the bf16 step -- the flash loss forward k_lbf_fwd + k_lbf_combine (csrc/logits_bf16.hip) and the fused
table updates k_tab16<EXTRA, KD> (csrc/table_update_sh.hip) and the theta-resident k_tab_upd<false, true, ...> (csrc/table_update.hip)
-- in the measure of oracle/x3_step_ref.py (imported, not copied: row_errors / quantity_errors / check / FACTOR / FLOOR are that
module's).  Test infrastructure: torch on the CPU only.

What makes a bf16 check tight is the decomposition OPERANDS EXACT, ARITHMETIC ROW-WISE:
  operands   the two bf16 operands are checked BITWISE against their definition (check_rep_bf: rep_bf = bf16(rep), round to nearest
             even, zero padded, in the plain or the distilled row layout; check_shadow: shadow[i, :H] = bf16(theta[i]), padding zero);
  reference_bf16(inp)   the float64 closed forms of x3_step_ref.reference() on THOSE operands: the logits, the target logit and the
             target row of dRep come from the shadow rows and rep_bf (k_lbf_combine<false>), the target term of the table gradient
             is wrow[b] * float(rep_bf[b]) (SH_TG_VAL), a distilled row's target term is rep_bf . O2 with O2 the teacher readout over
             the shadow rows; the input rows are the float32 dx rows times float32 sqrt(H).  The 2^-9 relative rounding of the operands is therefore
             NOT in the error: what is left is float32 accumulation, exp2 / log2, and the one rounding the kernels state -- p to bf16;
  emulate_bf16(inp, form)   that stated arithmetic in float32 (below); its error against reference_bf16 sets the bound of every
             quantity: max(FACTOR x emulated error, FLOOR), one-sided (see check_bf16).

The stated arithmetic (emulate_bf16):
  forward  S = rep_bf . E^T accumulated in float32 from bf16 operands.  Per item range (lbf_ranges: the 32-item blocks of the WHOLE
           catalog dealt to R ranges, a distilled row's blocks clipped to Np) an online max / sum-exp with the LAZY rescale of k_lbf_fwd:
           the running maximum only moves when a block's maximum exceeds it by more than 6 (log2 units), so p <= 2^6;
           p = exp2(fma(S, log2e, -m)), l += sum p in float32, p ROUNDED TO BF16, O += P^T . E in float32.  The ranges are merged with
           the factors exp2(pm - M), an empty range contributing 0; lse2 = M + log2 L, lse = lse2 / log2e, dRep = w (O / L - Et),
           rowloss = w (lse - rep_bf . Et).  A distilled row's Et is the teacher readout O2 = sum_j bf16(exp2(fma(t_j, log2e, -tlse2))) E_j.
  update   p = exp2(fma(S, log2e, off_b)), off = log2 w - lse2; in a distilled chunk the teacher's exp2(fma(t, log2e, log2 w - tlse2)) is
           subtracted FIRST and the items >= Np are zeroed; the result is rounded to bf16 and multiplied into rep_bf with float32
           accumulation over all batch rows ("sh": one accumulator per output; "resident": the two 32-row halves of every 64-row chunk
           apart, summed at the end).
  sparse   the input rows added, then the label terms subtracted, each in (id, position) list order (x3_step_ref._scatter_ordered's
           order); a split distillation's dense EXTRA rows -- the exact-f32 kernels' table gradient of the exemplar rows
           (x3_step_ref.emulate_f32) -- are added LAST, inside the optimiser phase.

Adam: the derived bounds of x3_step_ref.check_adam_* hold unchanged (CONTRACTED ADAM in that module: the bf16 kernels are not compiled
under fp contract(off)).  After the step the shadow must again be bf16(theta) bitwise, and the rows no launch owns bitwise untouched in
theta, m, v AND the shadow (x3_step_ref.check_untouched / check_range_untouched take the shadow as a fourth table).

Input families: BF16_CASES (the families of x3_step_ref.CASES that apply, at the mechanisms of THESE kernels) and the forms each runs in."""
import numpy as np
import torch

from . import x3_step_ref as X

LDR, FB = 168, 32                   # csrc/lbf_common.h, csrc/logits_bf16.hip
RESCALE_THR = 6.0
FORMS = ("sh", "resident", "kd_fast", "kd_split")
ParityError = X.ParityError


def _pad128(n):
    return (n + 127) // 128 * 128


def bf16r(x):
    """float32 -> bf16, round to nearest even (what `(bf16)x` compiles to on gfx950)."""
    return torch.as_tensor(x, dtype=torch.float32).detach().cpu().to(torch.bfloat16)


def _bits(t):
    return torch.as_tensor(t).detach().cpu().contiguous().view(torch.int16)


# =============================================================================================== operands, bitwise
def expected_rep_bf(rep, n_train, n_ex, kd):
    """[Bp, LDR] bf16: rows [0, n_train) -- and, in the distilled layout, rows [kd_row0, kd_row0 + n_ex), kd_row0 = n_train padded to
    128 -- hold bf16(rep) of the compact rep [n_train + n_ex, H]; columns >= H and every other row are zero (k_lbf_prep / k_lbf_prep_kd)."""
    rep = torch.as_tensor(rep, dtype=torch.float32).cpu()
    rows, total = X.step_rows(n_train, n_ex, kd)
    out = torch.zeros(total, LDR, dtype=torch.bfloat16)
    out[rows, :rep.shape[1]] = bf16r(rep)
    return out


def _raise_first(what, got, want):
    bad = torch.nonzero(got != want)
    if bad.numel():
        r, c = int(bad[0, 0]), int(bad[0, 1])
        raise ParityError("%s: row %d, column %d holds bits 0x%04x, expected 0x%04x (%d elements differ)"
                          % (what, r, c, int(got[r, c]) & 0xffff, int(want[r, c]) & 0xffff, bad.shape[0]))


def check_rep_bf(rep_bf_dev, rep, n_train, n_ex, kd):
    """The device's operand plane against expected_rep_bf, bitwise.  Returns the compact [n_train + n_ex, H] rows as float32."""
    want = expected_rep_bf(rep, n_train, n_ex, kd)
    got = torch.as_tensor(rep_bf_dev).detach().cpu().reshape(-1, LDR)
    if got.shape != want.shape:
        raise ParityError("rep_bf: %d rows, expected %d" % (got.shape[0], want.shape[0]))
    _raise_first("rep_bf", _bits(got), _bits(want))
    rows, _ = X.step_rows(n_train, n_ex, kd)
    return got[rows, :rep.shape[1]].float()


def expected_shadow(theta):
    theta = torch.as_tensor(theta, dtype=torch.float32).cpu()
    out = torch.zeros(theta.shape[0], LDR, dtype=torch.bfloat16)
    out[:, :theta.shape[1]] = bf16r(theta)
    return out


def check_shadow(shadow_dev, theta, what="shadow"):
    """shadow [>= V rows of LDR] against theta [V, H], bitwise: shadow[i, :H] == bf16(theta[i]), the padding columns and every row
    beyond the table zero.  Returns the table's shadow rows [V, H] as float32 (the GEMM operand)."""
    theta = torch.as_tensor(theta).detach().cpu()
    got = torch.as_tensor(shadow_dev).detach().cpu().reshape(-1, LDR)
    V = theta.shape[0]
    if got.shape[0] < V:
        raise ParityError("%s: %d rows, the table has %d" % (what, got.shape[0], V))
    want = torch.zeros(got.shape[0], LDR, dtype=torch.bfloat16)
    want[:V] = expected_shadow(theta)
    _raise_first(what, _bits(got), _bits(want))
    return got[:V, :theta.shape[1]].float()


def with_operands(inp, rep_bf=None, Esh=None):
    """inp of x3_step_ref.make_inputs plus the two bf16 operands as float32: rep_bf [B, H] (compact rows) and Esh [V, H] (the shadow
    rows of the whole table).  Default: rounded here from inp's rep / E0 (the host tests; the GPU tests pass the device's own)."""
    rep_bf = bf16r(inp["rep"]).float() if rep_bf is None else torch.as_tensor(rep_bf, dtype=torch.float32).cpu()
    Esh = bf16r(inp["E0"]).float() if Esh is None else torch.as_tensor(Esh, dtype=torch.float32).cpu()
    assert rep_bf.shape == inp["rep"].shape and Esh.shape == inp["E0"].shape
    return dict(inp, rep_bf=rep_bf, Esh=Esh)


# =============================================================================================== float64 reference
def split_inputs(inp):
    """A split distillation (Engine.kd_split without kd_fast): (the train rows -- bf16 flash kernels; every input position of the batch
    stays with them -- , the exemplar rows -- exact-f32 kernels on the float32 rep and table, no input positions)."""
    n, B = inp["n_train"], inp["B"]
    tr = dict(inp, rep=inp["rep"][:n], rep_bf=inp["rep_bf"][:n], B=n, y=inp["y"][:n], w=inp["w"][:n], tl=None, Np=0)
    ex = dict(inp, rep=inp["rep"][n:], rep_bf=inp["rep_bf"][n:], B=B - n, n_train=0, y=inp["y"][n:], w=inp["w"][n:],
              seq=torch.zeros(0, dtype=torch.int64), dx=torch.zeros(0, inp["H"]))
    return tr, ex


def reference_bf16(inp, form="sh"):
    """x3_step_ref.reference()'s closed forms and term sums in float64 on the device's bf16 operands.  form = "kd_split": the TRAIN rows'
    forward quantities, and the table gradient of the whole step: the train rows' on the bf16 operands plus the exemplar rows' on the
    float32 ones (term sums added column by column)."""
    on_bf = lambda i: dict(i, E0=i["Esh"], rep=i["rep_bf"])      # noqa: E731
    if form != "kd_split":
        return X.reference(on_bf(inp))
    tr, ex = split_inputs(inp)
    ref, rx = X.reference(on_bf(tr)), X.reference(ex)
    t_g = ref["t_g"] + rx["t_g"]
    return dict(ref, g=ref["g"] + rx["g"], t_g=t_g, s_g=t_g.max(-1).values)


# =============================================================================================== float32 emulation
def lbf_ranges(N, Bp):
    """ader_lbf_ranges: item ranges per 128-row chunk."""
    nblk, nchunk = (N + FB - 1) // FB, max(Bp // 128, 1)
    return max(min((512 // nchunk) // 8 * 8, (nblk + 7) // 8 * 8), 8)


def lbf_ranges_kd(N, Bp, kd_row0):
    return lbf_ranges(N, (Bp // 128 + (Bp - kd_row0) // 128) * 128)


def lbf_readout_ranges(N, Bp, kd_row0):
    nsm, nkd, R = Bp // 128, (Bp - kd_row0) // 128, lbf_ranges_kd(N, Bp, kd_row0)
    if nkd < 1:
        return R
    nblk = (N + FB - 1) // FB
    r2 = min(R + max(((512 - (nsm + nkd) * R) // nkd) // 8 * 8, 0), (nblk + 7) // 8 * 8)
    return max(r2, R)


_L2E = float(X.LOG2E)


def _fma(a, b, c):
    """fmaf(a, b, c) elementwise, b a float32 scalar: the product of two float32 is exact in float64, the sum is rounded to float64 and
    from there to float32 (a rare double rounding of half a float32 ulp aside)."""
    return (a.double() * b + torch.as_tensor(c).double()).float()


def _exp2(x):
    return torch.exp2(x.float())


def _flash_rows(S, E, lim, N, R, round_p=True):
    """k_lbf_fwd on rows whose softmax runs over the first `lim` items, then the merge of k_lbf_combine.  S [B, >= lim] float32 logits,
    E [N, H].  Returns M, L [B], O [B, H], parts (pm, pl [R, B])."""
    B, H = S.shape[0], E.shape[1]
    ninf = -float("inf")
    nblk_all = (N + FB - 1) // FB                      # the ranges partition the blocks of the WHOLE catalog
    per = (nblk_all + R - 1) // R
    blk_lim = -(-lim // FB)
    pm, pl, pO = torch.full((R, B), ninf), torch.zeros(R, B), torch.zeros(R, B, H)
    for r in range(R):
        m, l, O = torch.full((B,), ninf), torch.zeros(B), torch.zeros(B, H)
        for blk in range(r * per, min(blk_lim, r * per + per)):
            i0, i1 = blk * FB, min(blk * FB + FB, lim)
            s = S[:, i0:i1]
            t2 = s.max(-1).values * X.LOG2E
            m_new = torch.where(t2 > m + RESCALE_THR, t2, m)
            alpha = torch.where(torch.isinf(m), torch.zeros(B), _exp2(m - m_new))
            l, O, m = l * alpha, O * alpha[:, None], m_new
            p = _exp2(_fma(s, _L2E, -m[:, None]))
            l = l + p.sum(-1)
            O = O + (p.to(torch.bfloat16).float() if round_p else p) @ E[i0:i1]
        pm[r], pl[r], pO[r] = m, l, O
    M = pm.max(0).values
    sc = torch.where(torch.isinf(pm), torch.zeros(()), _exp2(pm - M[None, :]))       # an empty range contributes 0
    return M, (pl * sc).sum(0), (pO * sc[:, :, None]).sum(0), (pm, pl)


EMU_FAULTS = ("target_f32_rep", "p_f32", "no_zero_Np", "sub_after_pack")


def emulate_bf16(inp, form="sh", fault=None):
    """The kernels' stated arithmetic in float32 (the module docstring).  form: "sh" | "resident" (vanilla / one-hot replay), "kd_fast"
    (distilled, all rows on the flash kernels), "kd_split" (train rows here, the exemplar rows' table gradient from
    x3_step_ref.emulate_f32 added last).  fault (the planted-fault tests): 'target_f32_rep' -- the label term of the table gradient taken
    from the float32 rep; 'p_f32' -- p NOT rounded to bf16 in the forward; 'no_zero_Np' -- a distilled row's items >= Np not zeroed;
    'sub_after_pack' -- the teacher term subtracted after the bf16 pack.  Returns the outputs of x3_step_ref.emulate()."""
    assert form in FORMS and (fault is None or fault in EMU_FAULTS)
    if form == "kd_split":
        tr, ex = split_inputs(inp)
        out = emulate_bf16(tr, "sh", fault)
        return dict(out, g=out["g"] + X.emulate_f32(ex)["g"])
    N, B, H, n_train, tl = inp["N"], inp["B"], inp["H"], inp["n_train"], inp["tl"]
    E, R, w, y = inp["Esh"][1:N + 1], inp["rep_bf"], inp["w"], inp["y"]
    kd = tl is not None
    assert kd == (form == "kd_fast")
    S = R @ E.t()
    if kd:
        Np = inp["Np"]
        Bt, Bk = _pad128(n_train), _pad128(B - n_train)
        nr = lbf_ranges_kd(N, Bt + Bk, Bt)
        a = _flash_rows(S[:n_train], E, N, N, nr, fault != "p_f32")
        b = _flash_rows(S[n_train:], E, Np, N, nr, fault != "p_f32")
        M, L, O = torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]), torch.cat([a[2], b[2]])
    else:
        M, L, O, _ = _flash_rows(S, E, N, N, lbf_ranges(N, _pad128(B)), fault != "p_f32")
    lse2 = M + torch.log2(L)
    lse = lse2 / X.LOG2E
    Et = torch.zeros(B, H)
    hot = y > 0
    Et[hot] = E[y[hot] - 1]                                         # the shadow row of the label
    t2off = None
    if kd:
        # ader_row_lse (natural log, float32), then tlse2 = tlse * log2e (k_lbf_prep_kd)
        tm = tl.max(-1).values
        tlse2 = (tm + torch.log(torch.exp(tl - tm[:, None]).sum(-1))) * X.LOG2E
        # teacher readout: per range of the readout's own partition, plain sums (lbf_teacher_readout, k_lbf_combine)
        r2 = lbf_readout_ranges(N, Bt + Bk, Bt)
        per2 = ((N + FB - 1) // FB + r2 - 1) // r2
        pt = _exp2(_fma(tl, _L2E, -tlse2[:, None])).to(torch.bfloat16).float()
        O2 = torch.zeros(B - n_train, H)
        for r in range(r2):
            i0, i1 = min(r * per2 * FB, Np), min((r * per2 + per2) * FB, Np)
            if i1 > i0:
                O2 = O2 + pt[:, i0:i1] @ E[i0:i1]
        Et[n_train:] = O2
        t2off = torch.log2(w[n_train:]) - tlse2
    s_lab = (R * Et).sum(-1)
    rowloss = w * (lse - s_lab)
    drep = w[:, None] * (O / L[:, None] - Et)
    # ---- table update
    off = torch.log2(w) - lse2
    c = _exp2(_fma(S, _L2E, off[:, None]))
    if kd:
        tsub = _exp2(_fma(tl, _L2E, t2off[:, None]))
        if fault == "sub_after_pack":
            c[n_train:] = c[n_train:].to(torch.bfloat16).float()
        c[n_train:, :Np] -= tsub
        if fault != "no_zero_Np":
            c[n_train:, Np:] = 0.0
    cb = c.to(torch.bfloat16).float()
    if form == "resident":
        halves = [torch.zeros(N, H), torch.zeros(N, H)]
        for b0 in range(0, B, 64):
            for h in (0, 1):
                r0, r1 = b0 + 32 * h, min(b0 + 32 * h + 32, B)
                if r1 > r0:
                    halves[h] += cb[r0:r1].t() @ R[r0:r1]
        g = (halves[0] + halves[1]).numpy()
    else:
        g = (cb.t() @ R).numpy()
    g = X._scatter_ordered(g, inp)
    lab = (w[:, None] * (inp["rep"] if fault == "target_f32_rep" else R)).numpy()
    yn = y.numpy()
    for b in np.argsort(yn, kind="stable"):
        if yn[b] > 0:
            g[yn[b] - 1] -= lab[b]
    return dict(lse=lse, rowloss=rowloss, loss=rowloss.sum(), drep=drep, g=torch.from_numpy(g), c=cb, rep_q=R, parts=None, off=off)


def check_bf16(dev, inp, form="sh", ref=None, emu=None):
    """x3_step_ref.check of device outputs against reference_bf16 with the bound from emulate_bf16.  (kd_split: dev holds the TRAIN
    rows' lse / rowloss / drep, their loss, and the table gradient of the whole step.)
    The measure is ONE-SIDED: an output closer to the float64 reference than the emulation is never a fault -- a forward that kept p in
    float32 would pass.  The rounding of p is nevertheless pinned: it IS the emulated error of drep, and a bound computed without it is
    one that the stated arithmetic itself exceeds (tests/test_bf16_step_ref_host.py)."""
    ref = ref if ref is not None else reference_bf16(inp, form)
    emu = emu if emu is not None else emulate_bf16(inp, form)
    return X.check(dev, split_inputs(inp)[0] if form == "kd_split" else inp, ref=ref, emu=emu)


# =============================================================================================== Adam, shadow, untouched rows
def tile_is_misaligned(tile, H, base_bytes=0):
    """Whether the 64-row tile's first float of theta / m / v sits 8 bytes past a 16-byte boundary (the table starts 16-byte aligned at
    row 0 plus base_bytes): the kernels then peel `head` = 2 floats, and the flat [64 H] block ends in a 2-float vector."""
    return (base_bytes + 4 * H * (1 + 64 * tile)) % 16 != 0


UPDATE_FAULTS = ("head", "tail2", "shadow_straddle", "shadow_stale", "extra_beyond_N", "row_N1")


def update_emulate(theta0, m0, v0, sh0, g, N, k, fault=None, tile=1, extra=None):
    """TF ApplyAdam on rows 1..N (x3_step_ref.adam_emulate) and the shadow rebuilt from the updated rows, as full tables
    (theta, m, v [V, H] numpy; shadow [V, LDR] bf16).  g [N, H] float32.  Planted faults at 64-row tile `tile` (H % 4 == 2):
      'head'             the two peeled floats of the tile (its first row, columns 0 and 1) are left un-updated, shadow included;
      'tail2'            the 2-float vector that ends the tile's flat block (its last row, columns H-2, H-1) is dropped;
      'shadow_straddle'  the bf16 pair (p[2], p[3]) of the vector that crosses from the tile's second row into its third is written
                         behind the second row's end (columns H, H+1) instead of at the third row's columns 0, 1;
      'shadow_stale'     one shadow row of the tile keeps its old bits;
      'extra_beyond_N'   the optimiser phase of the tail tile runs over ALL its 64 rows with the dense EXTRA rows as their gradient
                         (extra [V, H], zero beyond N as the engine leaves it);
      'row_N1'           row N + 1 takes an update with a gradient of 1e-3."""
    assert fault is None or fault in UPDATE_FAULTS
    H = np.asarray(theta0).shape[1]
    th, m, v = X.adam_emulate(theta0, m0, v0, g, N, k, fault="row_N1" if fault == "row_N1" else None)
    t0 = [np.asarray(torch.as_tensor(t).numpy(), dtype=np.float32) for t in (theta0, m0, v0)]
    r_first, r_last = 64 * tile + 1, min(64 * tile + 64, N)
    if fault == "extra_beyond_N":
        V = th.shape[0]
        lo, hi = N + 1, min(((N + 63) // 64) * 64, V - 1)
        assert hi >= lo
        gx = np.asarray(torch.as_tensor(extra).numpy(), dtype=np.float32)[lo:hi + 1]
        th2, m2, v2 = X.adam_emulate(np.concatenate([t0[0][:1], t0[0][lo:hi + 1]]), np.concatenate([t0[1][:1], t0[1][lo:hi + 1]]),
                                     np.concatenate([t0[2][:1], t0[2][lo:hi + 1]]), gx, hi - lo + 1, k)
        th[lo:hi + 1], m[lo:hi + 1], v[lo:hi + 1] = th2[1:], m2[1:], v2[1:]
    if fault == "head":
        assert tile_is_misaligned(tile, H)
        for new, old in zip((th, m, v), t0):
            new[r_first, :2] = old[r_first, :2]
    if fault == "tail2":
        assert tile_is_misaligned(tile, H) and r_last == 64 * tile + 64
        for new, old in zip((th, m, v), t0):
            new[r_last, H - 2:] = old[r_last, H - 2:]
    sh = torch.as_tensor(sh0).detach().cpu().reshape(-1, LDR).clone()
    new_sh = expected_shadow(torch.from_numpy(th))
    hi = N + 1 if fault == "row_N1" else N
    if fault == "extra_beyond_N":
        hi = min(((N + 63) // 64) * 64, th.shape[0] - 1)
    sh[1:hi + 1] = new_sh[1:hi + 1]
    if fault == "shadow_straddle":
        # vectors start at the floats e = 2 + 4 t of the tile and H % 4 == 2: the end of the tile's row 1 (e = 2 H, a multiple of 4)
        # falls INSIDE the vector at e = 2 H - 2, which holds (row 1: H-2, H-1 | row 2: 0, 1)
        assert tile_is_misaligned(tile, H) and H % 4 == 2
        sh[r_first + 1, H:H + 2] = new_sh[r_first + 2, 0:2]
        sh[r_first + 2, 0:2] = torch.as_tensor(sh0).detach().cpu().reshape(-1, LDR)[r_first + 2, 0:2]
    if fault == "shadow_stale":
        sh[r_first + 5] = torch.as_tensor(sh0).detach().cpu().reshape(-1, LDR)[r_first + 5]
    return th, m, v, sh


def check_shadow_after(shadow_after, theta_after, shadow_before, N):
    """After the fused update, bitwise: shadow[1..N, :H] == bf16(theta_after), the padding columns of those rows still zero; every
    other shadow row (row 0, rows > N -- the rows of the last tile beyond the catalog among them -- and the rows beyond the table) is
    what it was.  Names the first row that is not."""
    sa = torch.as_tensor(shadow_after).detach().cpu().reshape(-1, LDR)
    sb = torch.as_tensor(shadow_before).detach().cpu().reshape(-1, LDR)
    want = sb.clone()
    want[1:N + 1] = expected_shadow(torch.as_tensor(theta_after).detach().cpu()[1:N + 1])
    _raise_first("shadow after the step (rows 1..%d rebuilt, the others untouched)" % N, _bits(sa), _bits(want))


def share_rule_passes(theta_a, theta_b, shadow_a, shadow_b, table_rows=4322):
    """The kernel-against-kernel measure of tests/test_gpu_parity.py (test_fused_table_adam_equals_unfused_step,
    test_both_bf16_update_forms_agree): 99.9 % of the parameters within 2e-6 and none beyond 1.1e-3; fewer than 1e-3 of the shadow
    elements different -- as shares of THAT test's tensors (N = 4321, H = 150: at least table_rows x H parameters, table_rows x 168
    shadow elements), applied to the differences of two tables of any size."""
    d = np.abs(np.asarray(theta_a, dtype=np.float64) - np.asarray(theta_b, dtype=np.float64))
    sa, sb = (torch.as_tensor(s).float().numpy() for s in (shadow_a, shadow_b))
    H = d.shape[1]
    return bool(np.sum(d >= 2e-6) < 1e-3 * table_rows * H and d.max() < 1.1e-3 and np.sum(sa != sb) < 1e-3 * table_rows * LDR)


NERR_BF16 = 6e-3        # tests/test_gpu_parity.py: every gradient tensor of the bf16 step within 6e-3 of its maximum


# =============================================================================================== range launches
def tile_ranges(N, W, item_num):
    """The 128-item tile ranges (tile_begin, tile_count) of W ranks of the row-sharded replicated update (Engine.shard_items // 128
    tiles each), and the table rows (1-based, inclusive; (1, 0): none) each launch may write."""
    S = -(-item_num // (128 * W)) * 128
    tiles = S // 128
    return [(r * tiles, tiles) for r in range(W)], X.shard_table_rows([(r * S, S) for r in range(W)], N)


# =============================================================================================== input families
def _forms(c, forms):
    return dict(c, forms=forms)


_UPD, _KDF, _KDS = ("sh", "resident"), ("kd_fast",), ("kd_fast", "kd_split")
# Numbers from the kernels: 64-row tiles (k_tab16, k_tab_upd), 32-item blocks dealt to >= 8 ranges and 128-row chunks (k_lbf_fwd), 64-row
# rep chunks of the update, rows padded to 128, 3 prefetched / 8 inline list entries, > 32 entries = heavy path, 256 entries per fetch.
# H = 150, 158, 10: H % 4 == 2 -- every tile starts 8 bytes past a 16-byte boundary (the peeled head, the 2-float tail, bf16 pairs that
# cross row ends); H = 64, 156: aligned.
BF16_CASES = (
    [_forms(X._BY_NAME["N%d" % n], _UPD) for n in (2, 63, 64, 65, 128, 129, 650)]
    # the catalog fills the table: the last tile's operand rows beyond it are read as zeros, there is no row N + 1
    + [_forms(X._case("N650_full", item_num=650), _UPD)]
    + [_forms(X._case("B%d" % b, B=b), _UPD) for b in (1, 64, 65, 128, 129)]
    # (H = 160, the padded width itself, is not a shape the engine takes -- hidden_units <= 159 --: 156 is the widest aligned one)
    + [_forms(X._case("H%d" % h, H=h), _UPD) for h in (158, 64, 156, 10)]
    + [_forms(X._BY_NAME["lists_records"], _UPD), _forms(X._BY_NAME["lists_hot"], _UPD), _forms(X._BY_NAME["onehot"], _UPD)]
    # every input position holds a LABEL of the batch: each row with sparse entries then carries a label term, which dominates its term
    # sum -- the family in which the operand of that term (SH_TG_VAL: rep_bf, not rep) is visible in g_sparse
    + [_forms(dict(X._case("label_rows"), label_rows=True), _UPD)]
    + [_forms(X._BY_NAME["kd_Np%d_ex%d" % k], f) for k, f in (((648, 70), _KDF), ((645, 70), _KDS), ((64, 70), _KDS), ((650, 70), _KDF),
                                                               ((648, 1), _KDF))]
    # a teacher CLOSE to the student (distillation from the previous period's model), one exemplar row beside 300 train rows: the
    # logit gradient of the distilled row is a small difference of two probabilities -- where the order "subtract, then round to bf16"
    # is visible in the table gradient (tests/test_bf16_step_ref_host.py)
    + [_forms(dict(X._case("kd_near_ex1", B=300, mode="kd", Np=648, n_ex=1, lam=0.7), near=True), _KDF)]
)
BF16_CASE_BY_NAME = {c["name"]: c for c in BF16_CASES}
BF16_RUNS = [(c["name"], f) for c in BF16_CASES for f in c["forms"]]
RANGE_RUNS = [(n, W) for n in ("N650", "N129") for W in (2, 3)]


def make_batch(case, seed=0):
    """x3_step_ref.make_batch; in the `label_rows` family every real input position is then redrawn from the batch's labels."""
    batch = X.make_batch(case, seed)
    if case.get("label_rows"):
        rs = np.random.RandomState(2000 + seed)
        seq = batch["seq"]
        redrawn = batch["pos"][rs.randint(0, len(batch["pos"]), size=seq.shape)]
        seq[...] = np.where(seq > 0, redrawn, 0)
    return batch


def set_near_teacher(case, batch, rep_ex, table, seed=0):
    """The `near` family: the teacher rows the batch's exemplar rows use are overwritten (in place) with the student's own logits on the
    bf16 operands -- rep_ex [n_ex, H] the exemplar rows' representations, table [V, H] -- plus 0.02 randn."""
    Np = case["Np"]
    g = torch.Generator().manual_seed(400 + seed)
    tl = bf16r(rep_ex).float() @ bf16r(table).float()[1:Np + 1].t() + 0.02 * torch.randn(case["n_ex"], Np, generator=g)
    batch["teacher"][batch["trow"]] = tl.numpy()


def host_inputs(case, seed=0):
    """(batch, inp): the case's batch and synthetic upstream tensors with the bf16 operands rounded from them."""
    batch = make_batch(case, seed)
    E0, rep, dx = X.synth_upstream(case, batch, seed)
    if case.get("near"):
        set_near_teacher(case, batch, rep[case["B"]:], E0, seed)
    return batch, with_operands(X.inputs_of(case, batch, E0, rep, dx))
