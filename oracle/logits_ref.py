"""Element-wise float64 reference of the dense logits (ader_logits_store: k_logits_tile<MODE_STORE>, logits.hip) and of the row
log-sum-exp (ader_row_lse: k_row_lse), with the measure their rounding error follows.  Test infrastructure: torch on the CPU only.

Every inference test takes Engine.logits as the truth and asserts bytes or integer counts against it; this module is what holds
that anchor to float64, ELEMENT BY ELEMENT:
  reference(rep, E, N)       s = rep . E[1..N]^T in float64 and its term sum t[b, n] = sum_k |rep[b, k] E[n, k]| -- the quantity the
                             rounding error of one output follows.
  emulate(rep, E, N)         the kernel's stated arithmetic: one float32 accumulator per output, acc = fmaf(e_k, r_k, acc) for k in
                             order (mma_tile on v_mfma_f32_16x16x4_f32; x3_step_ref._chain_mm, NOT a blocked sum).  The k steps beyond H
                             multiply staged zeros and add exactly nothing, so the chain runs over the H real columns.
  check_store(dev, ...)      every element on its own:  |dev - ref| / (t[b, n] + 2^-24 max t)  must stay within
                             max(FACTOR x the largest emulated error in that measure, FLOOR) -- x3_step_ref's bound, no new number.  A
                             wrong small element, a wrong row of one 64-row chunk or a wrong column of the last partial 64-item tile
                             is of order one in it, whatever the largest logit of the tensor is; a failure names (row, item), the
                             row's chunk and the item's tile.
  row_lse_reference / row_lse_emulate / check_row_lse
                             the float64 log-sum-exp of float32 rows; k_row_lse as written (256 strided partial maxima, the halving
                             tree, 256 strided partial sums of expf(x - m) in column order, the halving tree, m + logf(l)); judged in
                             the measure x3_step_ref uses for lse (s_lse = max(|lse|, 1)) with the same FACTOR / FLOOR.
The planted faults of tests/test_logits_ref_host.py are built from these pieces (FAULTS / plant)."""
import numpy as np
import torch

from .x3_step_ref import FACTOR, FLOOR, U24, ParityError, _chain_mm, row_errors

TI = 64          # items per tile (logit_tile.h)
TB = 64          # batch rows per chunk
LSE_THREADS = 256


def _f32(t):
    return torch.as_tensor(t).detach().to(torch.float32).cpu()


# =============================================================================================== dense logits
def reference(rep, E, N):
    """(s, t) float64 [B, N]: s = rep . E[1..N]^T and its term sum.  rep [>= B, H] (all its rows are used), E the table [>= N + 1, H]
    (row 0 = the padding item)."""
    r, e = _f32(rep).double(), _f32(E)[1:N + 1].double()
    return r @ e.t(), r.abs() @ e.abs().t()


def emulate(rep, E, N):
    """float32 [B, N]: the fmaf chain of mma_tile over k = 0 .. H - 1 in order, one accumulator per output."""
    return _chain_mm(_f32(rep), _f32(E)[1:N + 1].t())


def element_errors(x, s, t):
    """The measure: |x - s| / (t + 2^-24 max t), element by element (float64 [B, N])."""
    return (torch.as_tensor(x).detach().cpu().double() - s).abs() / (t + U24 * t.max())


def check_store(dev, rep, E, N, ref=None, emu=None):
    """dev [B, N] (device or emulated logits of rep [B, H] against items 1..N of E) -> (error, emulated error, bound), the maxima over
    the elements; raises ParityError naming the worst elements when one of them exceeds the bound (or is not finite)."""
    s, t = ref if ref is not None else reference(rep, E, N)
    emu = emu if emu is not None else emulate(rep, E, N)
    dev = torch.as_tensor(dev).detach().cpu()
    if tuple(dev.shape) != tuple(s.shape):
        raise ParityError("logits: shape %s, expected %s" % (tuple(dev.shape), tuple(s.shape)))
    e_dev, e_emu = element_errors(dev, s, t), element_errors(emu, s, t)
    base = float(e_emu.max())
    bound = max(FACTOR * base, FLOOR)
    bad = ~(e_dev <= bound)                                  # (a NaN is bad)
    if bool(bad.any()):
        order = torch.argsort(torch.where(torch.isnan(e_dev), torch.full_like(e_dev, float("inf")), e_dev).reshape(-1), descending=True)
        worst = []
        for i in order[:4].tolist():
            b, n = divmod(i, s.shape[1])
            if bool(bad[b, n]):
                worst.append("(row %d, item %d) chunk %d tile %d: %.3g" % (b, n + 1, b // TB, n // TI, float(e_dev[b, n])))
        raise ParityError("logits: %d of %d elements beyond bound %.3g (emulated %.3g); worst %s" % (
            int(bad.sum()), bad.numel(), bound, base, "; ".join(worst)))
    return float(e_dev.max()), base, bound


FAULTS = ("drop_last_kstep", "row_xor_64", "shift_last_tile", "bf16_operand", "small_element_64ulp")


def plant(fault, rep, E, N, emu=None, ref=None):
    """The emulated logits with one fault planted (the host tests; a fault a kernel of this shape could have):
      drop_last_kstep       the chain stops one k step (4 columns) short of ksteps = (H + 3) >> 2: the last H - 4 (ksteps - 1) real columns;
      row_xor_64            rows 64 .. 127 (chunk 1) computed from row b ^ 64 (chunk 0's operand tile staged for chunk 1);
      shift_last_tile       the columns of the last partial 64-item tile hold their right neighbour's logit (the last one its own);
      bf16_operand          rep rounded to bf16 before the chain;
      small_element_64ulp   ONE element, the smallest |logit| of the tensor, off by 64 units of ITS measure (64 * 2^-24 * t[b, n]: 64 float32
                            ulps of the sum the element rounds as).  64 ulps of the small value itself lie below what a CORRECT chain of H
                            fmaf may err by, so no float32-grade criterion rejects those.
    Returns (logits, where): where = (row lo, row hi, item lo, item hi), inclusive, 1-based items, of the faulted region."""
    rep, E = _f32(rep), _f32(E)
    B, H = rep.shape
    out = (emu if emu is not None else emulate(rep, E, N)).clone()
    if fault == "drop_last_kstep":
        keep = 4 * (((H + 3) >> 2) - 1)
        assert 0 < keep < H
        return emulate(rep[:, :keep], E[:, :keep], N), (0, B - 1, 1, N)
    if fault == "row_xor_64":
        assert B >= 128
        out[64:128] = out[0:64].clone()
        return out, (64, 127, 1, N)
    if fault == "shift_last_tile":
        t0 = (N - 1) // TI * TI
        assert N - t0 >= 2 and N % TI != 0
        out[:, t0:N - 1] = out[:, t0 + 1:N].clone()
        return out, (0, B - 1, t0 + 1, N - 1)
    if fault == "bf16_operand":
        return emulate(rep.to(torch.bfloat16).float(), E, N), (0, B - 1, 1, N)
    if fault == "small_element_64ulp":
        s, t = ref if ref is not None else reference(rep, E, N)
        i = int(torch.argmin(out.abs().reshape(-1)))
        b, n = divmod(i, N)
        out[b, n] = (out[b, n].double() + 64 * U24 * t[b, n]).float()
        return out, (b, b, n + 1, n + 1)
    raise ValueError(fault)


# =============================================================================================== row log-sum-exp
def row_lse_reference(x, ncols):
    """float64 [R]: log sum exp over the first ncols columns of the float32 rows x [R, >= ncols]."""
    return torch.logsumexp(_f32(x)[:, :ncols].double(), -1)


def _halve(red, op):
    """The halving tree of k_row_lse over red [R, 256]: red[i] = op(red[i], red[i + s]) for i < s, s = 128 .. 1 -> red[:, 0]."""
    red = red.clone()
    s = LSE_THREADS // 2
    while s > 0:
        red[:, :s] = op(red[:, :s], red[:, s:2 * s])
        s >>= 1
    return red[:, 0]


def row_lse_emulate(x, ncols, fault=None):
    """float32 [R]: k_row_lse as written.  Thread i holds the maximum of columns i, i + 256, ..; the tree gives m; thread i then sums
    expf(x - m) over its columns in order (float32); the tree gives l; out = m + logf(l).  A column a thread does not have is -inf
    here: fmaxf ignores it and expf gives an exact 0.
    fault (the host tests): "max_short" -- the maximum taken over ncols - 1 columns; "drop_partial" -- thread 255's sum left out."""
    x = _f32(x)[:, :ncols]
    R = x.shape[0]
    steps = (ncols + LSE_THREADS - 1) // LSE_THREADS
    p = torch.full((R, steps * LSE_THREADS), -float("inf"))
    p[:, :ncols] = x
    p = p.reshape(R, steps, LSE_THREADS)
    pm = p
    if fault == "max_short":
        pm = p.clone().reshape(R, -1)
        pm[:, ncols - 1] = -float("inf")
        pm = pm.reshape(R, steps, LSE_THREADS)
    m = _halve(pm.max(1).values, torch.maximum)
    part = torch.zeros(R, LSE_THREADS)
    for k in range(steps):
        part = part + torch.exp(p[:, k] - m[:, None])
    if fault == "drop_partial":
        part[:, LSE_THREADS - 1] = 0.0
    return m + torch.log(_halve(part, torch.add))


def check_row_lse(dev, x, ncols, ref=None, emu=None):
    """dev [R] against the float64 log-sum-exp of x[:, :ncols] in x3_step_ref's lse measure (per row, |dev - ref| / (max(|ref|, 1) +
    2^-24 max of those)) -> (error, emulated error, bound); raises ParityError naming the worst rows."""
    ref = ref if ref is not None else row_lse_reference(x, ncols)
    emu = emu if emu is not None else row_lse_emulate(x, ncols)
    scale = ref.abs().clamp_min(1.0)
    e_dev, e_emu = row_errors(torch.as_tensor(dev).detach().cpu(), ref, scale), row_errors(emu, ref, scale)
    base = float(e_emu.max())
    bound = max(FACTOR * base, FLOOR)
    bad = ~(e_dev <= bound)
    if bool(bad.any()):
        rows = torch.nonzero(bad).reshape(-1)[:4].tolist()
        raise ParityError("row_lse: %d of %d rows beyond bound %.3g (emulated %.3g); rows %s" % (
            int(bad.sum()), bad.numel(), bound, base, ", ".join("%d (%.3g)" % (r, float(e_dev[r])) for r in rows)))
    return float(e_dev.max()), base, bound


# =============================================================================================== operands of the tests
def operands(B, N, H, seed, rows=None, item_num=None):
    """rep ~ N(0, 1) [rows or B, H] and the table E ~ 0.05 N(0, 1) [item_num or N + 1, H], seeded; float32."""
    g = torch.Generator().manual_seed(seed)
    rep = torch.randn(rows or B, H, generator=g)
    E = 0.05 * torch.randn(item_num or N + 1, H, generator=g)
    return rep, E


def format_line(name, res):
    err, base, bound = res
    return "%-40s device %.3e  emulated %.3e  ratio %.2fx  bound %.3e" % (name, err, base, err / max(base, 1e-300), bound)


def stable_ranks(logits, target):
    """0-based rank of item target[b] (1-based) in row b under (score descending, item id ascending): the count ader_rank_targets
    states, on the given float32 bytes.  numpy int64 [B]."""
    lg = np.asarray(logits, dtype=np.float32)
    tgt = np.asarray(target, dtype=np.int64) - 1
    tl = lg[np.arange(lg.shape[0]), tgt][:, None]
    idx = np.arange(lg.shape[1])[None, :]
    return ((lg > tl) | ((lg == tl) & (idx < tgt[:, None]))).sum(1)
