"""Row-wise float64 reference of the x3 loss forward (k_lx3p / k_lx3r + the merge) and of the fused table update (k_tab32x3),
with the measure their rounding error follows.  Test infrastructure: torch on the CPU only.

Three things live here:
  reference(inp)   the closed forms of ADER.py:91-93 / 126-137 in float64 from the kernels' own inputs (rep, the table, the
                   per-position gradient rows, labels / teacher rows), and beside every output its TERM SUM: the same expression with
                   every term replaced by its absolute value.  Errors are measured row by row as
                       max_c |x - ref| / (term_sum_row + 2^-24 max_rows term_sum)
                   -- the denominator rounding error follows.  A missing or mis-scaled term is of order one in it, and a small row
                   (one that only the gradient GEMM writes: 99.8 % of the table) cannot hide behind a large one.
  emulate(inp)     the kernels' stated arithmetic in float32 on the CPU: operands split into bf16 hi + lo, a product = hi.hi + lo.hi +
                   hi.lo accumulated in float32, exp2 / log2 in float32, the sparse rows added in the documented order (dense tile,
                   input positions in position order, label terms subtracted).  Its error against reference() is what a CORRECT
                   float32-grade computation costs on these inputs; it comes from the reference alone.
  check(dev, inp)  device (or emulated) outputs against reference(): each quantity must stay within
                   max(8 x the emulated error of that quantity on the same inputs, 16 * 2^-24).  8 covers summation order, the flash
                   rescaling and the hardware exp2; the floor covers inputs on which the emulation happens to be nearly exact.
The Adam half needs no measurement: its bounds are float32 rounding bounds of tf.train.AdamOptimizer's three lines (check_adam_*).

The input families of tests/test_gpu_x3_rowwise.py are built here too (CASES / make_batch), so that the host tests assert their
conditions -- enough rows that ONLY the gradient GEMM writes -- on the very inputs the GPU tests run."""
import numpy as np
import torch

U24 = 2.0 ** -24
FACTOR = 8.0                    # bound = max(FACTOR x emulated error, FLOOR)
FLOOR = 16 * U24
LOG2E = np.float32(1.4426950408889634)
TI = 64                         # table rows per tile of k_tab32x3


# =============================================================================================== inputs
def step_weights(n_train, n_ex, lambda_):
    """Per-row loss weights as the engine hands them to the kernels (backward.py: w_train, w_ex; C floats)."""
    w = np.empty(n_train + n_ex, dtype=np.float32)
    w[:n_train] = np.float32(1.0 / max(n_train, 1))
    if n_ex:
        w[n_train:] = np.float32(lambda_ / n_ex)
    return torch.from_numpy(w)


def make_inputs(E0, rep, seq, dx, N, n_train, pos, *, ex_pos=None, teacher_rows=None, lambda_=0.0):
    """The inputs of reference() / emulate().  E0 [V,H] the table before the step, rep [B,H], seq [B,T] ids (0 = padding),
    dx [B*T,H] per-position gradient rows of the input embeddings, pos [n_train] labels; exemplar rows are one-hot (ex_pos [n_ex])
    or distilled (teacher_rows [n_ex,Np]: the teacher logits of each exemplar row, already gathered)."""
    E0, rep, dx = (torch.as_tensor(t, dtype=torch.float32).cpu() for t in (E0, rep, dx))
    B, H = rep.shape
    n_ex = B - n_train
    y = torch.zeros(B, dtype=torch.int64)
    y[:n_train] = torch.as_tensor(np.asarray(pos)).long()
    tl = None
    if n_ex and teacher_rows is not None:
        tl = torch.as_tensor(teacher_rows, dtype=torch.float32).cpu()
        assert tl.shape[0] == n_ex and tl.shape[1] <= N
    elif n_ex:
        y[n_train:] = torch.as_tensor(np.asarray(ex_pos)).long()
    seq = torch.as_tensor(np.asarray(seq)).long().reshape(-1)
    assert dx.shape == (seq.numel(), H) and int(seq.max()) <= N and int(y.max()) <= N
    return dict(E0=E0, rep=rep, seq=seq, dx=dx, N=int(N), H=H, B=B, n_train=int(n_train), y=y, tl=tl,
                Np=(tl.shape[1] if tl is not None else 0), w=step_weights(n_train, n_ex, lambda_),
                sqrtH=float(np.sqrt(np.float32(H))))


def dense_only_rows(inp):
    """[N] bool: table rows 1..N that no input position and no label touches -- the gradient GEMM alone writes them."""
    touched = torch.zeros(inp["N"] + 1, dtype=torch.bool)
    touched[inp["seq"]] = True
    touched[inp["y"]] = True
    return ~touched[1:]


# =============================================================================================== float64 reference
def loss_tail_terms(inp, dt=torch.float64):
    """(valid [B,N] columns of each row's softmax, target distribution [B,N]) of ADER.py:93 / 126-137."""
    B, N, n_train, tl = inp["B"], inp["N"], inp["n_train"], inp["tl"]
    valid = torch.ones(B, N, dtype=torch.bool)
    tgt = torch.zeros(B, N, dtype=dt)
    hot = inp["y"] > 0
    tgt[torch.nonzero(hot).reshape(-1), inp["y"][hot] - 1] = 1.0
    if tl is not None:
        Np = inp["Np"]
        valid[n_train:, Np:] = False                       # sliced BEFORE the softmax (ADER.py:132-137)
        tgt[n_train:, :Np] = torch.softmax(tl.to(dt), -1)
    return valid, tgt


def reference(inp):
    """Closed forms in float64 and their term sums.  Returns a dict: lse, rowloss [B]; loss; drep [B,H]; g [N,H] (table rows 1..N);
    c [B,N] the logit gradient; s_lse, s_rowloss [B], s_loss, s_drep [B], s_g [N] the term sums."""
    dt = torch.float64
    N = inp["N"]
    E, rep, w = inp["E0"][1:N + 1].to(dt), inp["rep"].to(dt), inp["w"].to(dt)
    valid, tgt = loss_tail_terms(inp)
    s = rep @ E.t()
    sm = s.masked_fill(~valid, -float("inf"))
    lse = torch.logsumexp(sm, -1)
    p = torch.exp(sm - lse[:, None])
    tterm = (tgt * s).sum(-1)
    rowloss = w * (lse - tterm)
    c = w[:, None] * (p - tgt)
    drep = c @ E
    ids = inp["seq"]
    real = ids > 0
    dxs = inp["dx"].to(dt)[real] * inp["sqrtH"]
    g = c.t() @ rep
    g.index_add_(0, ids[real] - 1, dxs)
    s_g = c.abs().t() @ rep.abs()
    s_g.index_add_(0, ids[real] - 1, dxs.abs())
    s_rowloss = w.abs() * (lse.abs() + tterm.abs())
    return dict(lse=lse, rowloss=rowloss, loss=rowloss.sum(), drep=drep, g=g, c=c,
                s_lse=lse.abs().clamp_min(1.0), s_rowloss=s_rowloss, s_loss=s_rowloss.sum(),
                s_drep=(c.abs() @ E.abs()).max(-1).values, s_g=s_g.max(-1).values)


def row_errors(x, ref, scale):
    """The measure: per row, max_c |x - ref| / (scale_row + 2^-24 max_rows scale)."""
    d = (torch.as_tensor(x).to(torch.float64) - ref).abs()
    if d.dim() == 2:
        d = d.max(-1).values
    scale = torch.as_tensor(scale, dtype=torch.float64)
    return d / (scale + U24 * scale.max())


# =============================================================================================== float32 emulation
def _split(x):
    hi = x.to(torch.bfloat16).float()
    return hi, (x - hi).to(torch.bfloat16).float()


def _x3mm(A, B):
    """A @ B as the x3 kernels form it: bf16 hi/lo splits, lo.hi + hi.lo + hi.hi, float32 accumulation."""
    ah, al = _split(A)
    bh, bl = _split(B)
    return (al @ bh + ah @ bl) + ah @ bh


def emulate(inp, chunk=None, ncol=None):
    """The kernels' arithmetic in float32.  chunk: accumulate the gradient GEMM in batch-row chunks of that size (the device: 32).
    ncol [B]: override of the number of softmax columns per row (the planted-fault tests).  Returns the outputs of reference() in
    float32 (lse, rowloss, loss, drep, g) plus c, the logit gradient the table update formed, and rep_q = rep_hi + rep_lo."""
    f32 = torch.float32
    N, B, n_train, tl = inp["N"], inp["B"], inp["n_train"], inp["tl"]
    E, rep, w, y = inp["E0"][1:N + 1], inp["rep"], inp["w"], inp["y"]
    l2e = torch.tensor(LOG2E)
    valid, _ = loss_tail_terms(inp, f32)
    if ncol is not None:
        valid = torch.arange(N)[None, :] < torch.as_tensor(ncol)[:, None]
    s2 = (_x3mm(rep, E.t().contiguous()) * l2e).masked_fill(~valid, -float("inf"))
    M = s2.max(-1).values
    pun = torch.exp2(s2 - M[:, None])
    L = pun.sum(-1)
    lse2 = M + torch.log2(L)
    lse = lse2 / l2e
    Et = torch.zeros_like(rep)
    hot = y > 0
    Et[hot] = E[y[hot] - 1]                                      # target row from the fp32 operands (k_lbf_combine<X3>)
    toff = None
    if tl is not None:
        Np = inp["Np"]
        t2 = tl * l2e
        tM = t2.max(-1).values
        tlse2 = tM + torch.log2(torch.exp2(t2 - tM[:, None]).sum(-1))
        Et[n_train:] = _x3mm(torch.exp2(t2 - tlse2[:, None]), E[:Np])          # teacher readout O2
        toff = torch.log2(w[n_train:]) - tlse2
    s_lab = (rep * Et).sum(-1)
    rowloss = w * (lse - s_lab)
    drep = w[:, None] * (_x3mm(pun, E) / L[:, None] - Et)
    # ---- table update: p = w softmax = exp2(s log2e + off), off = log2 w - lse2; distilled rows minus w softmax(t)
    off = torch.log2(w) - lse2
    c = torch.exp2(s2 + off[:, None])
    if tl is not None:
        c[n_train:, :Np] -= torch.exp2(t2 + toff[:, None])
        c[n_train:, Np:] = 0.0
    rh, rl = _split(rep)
    rep_q = rh + rl
    if chunk:
        g = torch.zeros(N, inp["H"], dtype=f32)
        for b0 in range(0, B, chunk):
            g += _x3mm(c[b0:b0 + chunk].t().contiguous(), rep[b0:b0 + chunk])
    else:
        g = _x3mm(c.t().contiguous(), rep)
    g = g.numpy()
    # sparse rows in (id, position) order: input positions added, then label terms subtracted; two rounded operations each
    ids = inp["seq"].numpy()
    dxs = (inp["dx"] * torch.tensor(np.float32(inp["sqrtH"]))).numpy()
    for k in np.argsort(ids, kind="stable"):
        if ids[k] > 0:
            g[ids[k] - 1] += dxs[k]
    lab = (w[:, None] * rep_q).numpy()
    yn = y.numpy()
    for b in np.argsort(yn, kind="stable"):
        if yn[b] > 0:
            g[yn[b] - 1] -= lab[b]
    return dict(lse=lse, rowloss=rowloss, loss=rowloss.sum(), drep=drep, g=torch.from_numpy(g), c=c, rep_q=rep_q)


# =============================================================================================== check
QUANTITIES = ("lse", "rowloss", "loss", "drep", "g_dense", "g_sparse")


def quantity_errors(x, ref, dense):
    """Per quantity: the row errors of outputs x against the reference."""
    eg = row_errors(x["g"], ref["g"], ref["s_g"])
    loss_err = (torch.as_tensor(x["loss"]).double().reshape(()) - ref["loss"]).abs() / ref["s_loss"]
    return {"lse": row_errors(x["lse"], ref["lse"], ref["s_lse"]),
            "rowloss": row_errors(x["rowloss"], ref["rowloss"], ref["s_rowloss"]),
            "loss": loss_err.reshape(1),
            "drep": row_errors(x["drep"], ref["drep"], ref["s_drep"]),
            "g_dense": torch.where(dense, eg, torch.zeros_like(eg)),
            "g_sparse": torch.where(~dense, eg, torch.zeros_like(eg))}


class ParityError(AssertionError):
    pass


def check(dev, inp, ref=None, emu=None):
    """dev: dict lse [B], rowloss [B], loss, drep [B,H], g [N,H] in the compact row numbering.  Returns {quantity: (error, emulated
    error, bound)}; raises ParityError naming the quantity and its worst rows when an error exceeds its bound."""
    ref = ref if ref is not None else reference(inp)
    emu = emu if emu is not None else emulate(inp)
    dense = dense_only_rows(inp)
    e_dev, e_emu = quantity_errors(dev, ref, dense), quantity_errors(emu, ref, dense)
    out, bad = {}, []
    for q in QUANTITIES:
        err, base = float(e_dev[q].max()), float(e_emu[q].max())
        bound = max(FACTOR * base, FLOOR)
        out[q] = (err, base, bound)
        if not err <= bound:
            worst = torch.argsort(e_dev[q], descending=True)[:4]
            first = 1 if q.startswith("g_") else 0              # table rows are reported by item id
            bad.append("%s: %.3g > bound %.3g (emulated %.3g); worst rows %s" % (
                q, err, bound, base, ", ".join("%d (%.3g)" % (int(i) + first, float(e_dev[q][i])) for i in worst)))
    if bad:
        raise ParityError("; ".join(bad))
    return out


def format_ratios(res):
    """One line: device error / emulated error per quantity (and the error itself)."""
    return "  ".join("%s %.2fx (%.2e)" % (q, e / max(b, 1e-300), e) for q, (e, b, _) in res.items())


# =============================================================================================== Adam
def adam_consts(lr, b1p, b2p, beta1=0.9, beta2=0.999, eps=1e-8):
    """lr_t, 1 - beta1, 1 - beta2, eps as the float32 values the kernel receives (engine/update.py:_lr_t, oracle.TFAdam)."""
    lr_t = np.float32(lr) * np.sqrt(np.float32(1) - np.float32(b2p)) / (np.float32(1) - np.float32(b1p))
    return dict(lr_t=float(np.float32(lr_t)), omb1=float(np.float32(1) - np.float32(beta1)),
                omb2=float(np.float32(1) - np.float32(beta2)), eps=float(np.float32(eps)))


def adam_emulate(theta0, m0, v0, g, N, k, fault=None):
    """TF ApplyAdam on table rows 1..N in float32 (the kernel's three lines).  fault: 'eps_in_sqrt' | 'v_from_old_m' | 'row_N1'
    (the planted-fault tests).  Returns new (theta, m, v), full tables."""
    th, m, v = (np.array(torch.as_tensor(t).numpy(), dtype=np.float32, copy=True) for t in (theta0, m0, v0))
    g = np.asarray(torch.as_tensor(g).numpy(), dtype=np.float32)
    lr_t, omb1, omb2, eps = (np.float32(k[x]) for x in ("lr_t", "omb1", "omb2", "eps"))
    hi = N + 2 if fault == "row_N1" else N + 1
    if hi > N + 1:
        g = np.concatenate([g, np.full((1, g.shape[1]), 1e-3, np.float32)])
    r = slice(1, hi)
    gg = m[r].copy() if fault == "v_from_old_m" else g
    m[r] += (g - m[r]) * omb1
    v[r] += (gg * gg - v[r]) * omb2
    den = np.sqrt(v[r] + eps) if fault == "eps_in_sqrt" else np.sqrt(v[r]) + eps
    th[r] -= (m[r] * lr_t) / den
    return th, m, v


def _f64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def _worst(name, excess):
    i = int(torch.argmax(excess))
    return "%s: element (row %d, col %d) exceeds its bound by %.3g" % (name, i // excess.shape[1], i % excess.shape[1], float(excess.max()))


def check_theta(theta0, theta1, m1, v1, N, k):
    """Always: theta' against theta0 - u, u = lr_t m' / (sqrt(v') + eps) from the device's own m', v':
    |theta' - (theta0 - u)| <= 2^-23 |theta0| + 2e-6 |u|  (one float32 subtraction; 2e-6 = five times the kernel's statement of its
    hardware sqrt / rcp: < 4e-7 of the update)."""
    r = slice(1, N + 1)
    t0, t1, m1, v1 = _f64(theta0)[r], _f64(theta1)[r], _f64(m1)[r], _f64(v1)[r]
    u = k["lr_t"] * m1 / (v1.sqrt() + k["eps"])
    excess = (t1 - (t0 - u)).abs() - (2.0 ** -23 * t0.abs() + 2e-6 * u.abs())
    if float(excess.max()) > 0:
        raise ParityError(_worst("theta", excess))


def check_adam_zero(theta0, theta1, m1, v1, N, k):
    """From zero Adam state: g_dev = m'/omb1 and |v' - omb2 g_dev^2| <= 2^-21 g_dev^2.  Held tighter where float32 is normal:
    v' = omb2 g^2 costs two roundings (three with g_dev's own), so the error is within 2^-21 of omb2 g_dev^2 ITSELF, plus 2^-126 for
    a result in the subnormal range -- the smaller of the two bounds applies.  Returns g_dev [N,H] (float64)."""
    r = slice(1, N + 1)
    m1r, v1r = _f64(m1)[r], _f64(v1)[r]
    g = m1r / k["omb1"]
    bound = torch.minimum(2.0 ** -21 * g * g, 2.0 ** -21 * k["omb2"] * g * g + 2.0 ** -126)
    excess = (v1r - k["omb2"] * g * g).abs() - bound
    if float(excess.max()) > 0:
        raise ParityError(_worst("v (zero state)", excess))
    check_theta(theta0, theta1, m1, v1, N, k)
    return g


def check_adam_preloaded(theta0, m0, v0, theta1, m1, v1, g, N, k):
    """From preloaded state, elementwise in float64 with the device's gradient g [N,H]:
    |m' - (m0 + (g - m0) omb1)| <= 2^-21 (|m0| + |g|),  |v' - (v0 + (g^2 - v0) omb2)| <= 2^-21 (v0 + g^2)."""
    r = slice(1, N + 1)
    m0r, v0r, m1r, v1r, g = _f64(m0)[r], _f64(v0)[r], _f64(m1)[r], _f64(v1)[r], _f64(g)
    ex_m = (m1r - (m0r + (g - m0r) * k["omb1"])).abs() - 2.0 ** -21 * (m0r.abs() + g.abs())
    ex_v = (v1r - (v0r + (g * g - v0r) * k["omb2"])).abs() - 2.0 ** -21 * (v0r + g * g)
    if float(ex_m.max()) > 0:
        raise ParityError(_worst("m (preloaded)", ex_m))
    if float(ex_v.max()) > 0:
        raise ParityError(_worst("v (preloaded)", ex_v))
    check_theta(theta0, theta1, m1, v1, N, k)


def check_untouched(before, after, N):
    """Rows 0 and > N of theta, m and v must be BITWISE what they were (before / after: triples of full [V,H] tables)."""
    for name, b, a in zip(("theta", "m", "v"), before, after):
        b = torch.as_tensor(b).detach().cpu().contiguous().view(torch.int32)
        a = torch.as_tensor(a).detach().cpu().contiguous().view(torch.int32)
        for lo, hi in ((0, 1), (N + 1, b.shape[0])):
            if not torch.equal(b[lo:hi], a[lo:hi]):
                row = lo + int(torch.nonzero((b[lo:hi] != a[lo:hi]).any(-1))[0])
                raise ParityError("%s: row %d is outside 1..%d and was written" % (name, row, N))


# =============================================================================================== input families
def _pool(N):
    """Ordinary ids: multiples of 4, so that three rows in four stay free of sparse entries (in a row with sparse entries the dense
    term is masked by them: a 2^-10 scale fault of the GEMM measured 4e-6 there against 4e-4 in a dense-only row)."""
    p = np.arange(4, N + 1, 4)
    return p if len(p) else np.array([N])


def _case(name, N=650, B=70, H=150, mode="vanilla", n_ex=0, Np=0, lam=0.0, plant=None, item_num=None):
    return dict(name=name, N=N, B=B, H=H, mode=mode, n_ex=n_ex, Np=Np, lam=lam, plant=plant, item_num=item_num or max(N + 50, 700), T=8)


# One family per mechanism, the others at their base value (H = 150, B = 70 train rows, N = 650).  Numbers from
# table_update_x3.hip: 64-row tiles in pairs, 32-row rep chunks, rows padded to 128, > 32 list entries = heavy path, 8 inline entries.
CASES = (
    [_case("N%d" % n, N=n) for n in (2, 63, 64, 65, 128, 129, 650)]
    + [_case("B%d" % b, B=b) for b in (1, 32, 33, 128, 129, 1153)]
    + [_case("lists_records", B=300, plant="records"), _case("lists_hot", B=300, plant="hot")]
    + [_case("onehot", B=53, n_ex=17, mode="onehot", lam=0.6)]          # 70 rows, a quarter of them exemplars
    + [_case("kd_Np%d_ex%d" % (np_, ne), mode="kd", Np=np_, n_ex=ne, lam=0.7)
       for np_, ne in ((648, 70), (650, 70), (64, 70), (130, 70), (645, 70), (648, 1), (645, 129), (650, 129))]
    + [_case("H%d" % h, H=h) for h in (64, 158, 10)]
)
CASE_IDS = [c["name"] for c in CASES]


def make_batch(case, seed=0):
    """The batch of a case: dict seq [B_all,T] int32 (train rows first), pos [B], ex_pos [n_ex] | teacher [n_ex+9,Np] + trow [n_ex]."""
    rs = np.random.RandomState(1000 + seed)
    N, B, T, n_ex = case["N"], case["B"], case["T"], case["n_ex"]
    Ba = B + n_ex
    pool = _pool(N)
    seq = np.zeros((Ba, T), dtype=np.int32)
    pos = pool[rs.randint(0, len(pool), size=B)].astype(np.int32)
    out = dict(seq=seq, pos=pos, ex_pos=None, teacher=None, trow=None)
    if case["plant"] is None:
        for b in range(Ba):
            ln = int(rs.randint(1, T + 1))
            seq[b, T - ln:] = pool[rs.randint(0, len(pool), size=ln)]
    else:
        # tiles (64 ids each, tile 10 = ids 641..650) are given their list lengths exactly: ordinary rows hold ONE real position
        quiet = {"records": 6, "hot": 7}[case["plant"]]             # ordinary ids live in tiles quiet..9
        pool = pool[(pool - 1) // TI >= quiet]
        pool = pool[(pool - 1) // TI <= 9]
        seq[:, T - 1] = pool[rs.randint(0, len(pool), size=Ba)]
        pos[:] = pool[rs.randint(0, len(pool), size=B)]
        if case["plant"] == "records":
            plan = [(5, 8),         # tile 0: 8 entries = the inline record exactly full
                    (70, 9),        # tile 1: 9 = one entry beyond it (from the global list)
                    (133, 32),      # tile 2: 32 = the most the light path takes
                    (197, 33),      # tile 3: 33 = heavy path
                    (261, 40), (262, 3), (330, 40),     # tiles 4 and 5: hot ids in both tiles of one pair
                    (645, 50), (650, 2)]                # tail tile (10 rows): a hot id, and the table's last row
            labels = []
        else:
            plan = [(77, 600),                          # one id in 600 positions (several 256-entry fetches) ...
                    (400, 250), (401, 20)]              # tile 6: its list exceeds 256 entries, id 401's run straddles entry 256
            labels = [(77, 120),                        # ... and 120 labels
                      (200, 40)]                        # tile 3: heavy in the label list only
        # dealt to the rows round-robin from the right, so that every row stays left-padded like a real session
        planted = rs.permutation(np.repeat([i for i, _ in plan], [c for _, c in plan]))
        assert len(planted) <= (T - 1) * Ba
        for i, idv in enumerate(planted):
            seq[i % Ba, T - 2 - i // Ba] = idv
        k = 0
        for idv, cnt in labels:
            pos[k:k + cnt] = idv
            k += cnt
    if case["mode"] == "onehot":
        out["ex_pos"] = pool[rs.randint(0, len(pool), size=n_ex)].astype(np.int32)
    elif case["mode"] == "kd":
        out["teacher"] = (rs.standard_normal((n_ex + 9, case["Np"])) * 2).astype(np.float32)
        out["trow"] = rs.permutation(n_ex + 9)[:n_ex].astype(np.int32)
    return out


def synth_upstream(case, batch, seed=0):
    """Host stand-ins for what the device's upstream hands the two kernels: a table (0.05 randn, the tests' initialisation), LayerNorm-
    sized representations and per-position gradient rows of the size a step produces (zero at the padding)."""
    g = torch.Generator().manual_seed(77 + seed)
    V, H = case["item_num"] + 1, case["H"]
    Ba = batch["seq"].shape[0]
    E0 = torch.randn(V, H, generator=g) * 0.05
    rep = torch.randn(Ba, H, generator=g) * 1.1 + 0.1
    dx = torch.randn(Ba * case["T"], H, generator=g) * (2e-3 / max(case["B"], 1))
    dx[torch.from_numpy(batch["seq"].reshape(-1) == 0)] = 0.0
    return E0, rep, dx


def inputs_of(case, batch, E0, rep, dx):
    tr = None
    if batch["teacher"] is not None:
        tr = torch.as_tensor(batch["teacher"]).cpu()[torch.as_tensor(batch["trow"]).long()]
    return make_inputs(E0, rep, batch["seq"], dx, case["N"], case["B"], batch["pos"], ex_pos=batch["ex_pos"], teacher_rows=tr,
                       lambda_=case["lam"])


def dense_only_condition(inp):
    """The condition on the inputs of every family: at least half of the table rows, and at least one row of every 16-row slice (a
    wave's rows) of the first tile, a middle tile and the tail tile, are dense-only.  Returns a complaint or None."""
    d = dense_only_rows(inp)
    N = inp["N"]
    if 2 * int(d.sum()) < N:
        return "only %d of %d rows are dense-only" % (int(d.sum()), N)
    tiles = (N + TI - 1) // TI
    for t in sorted({0, tiles // 2, tiles - 1}):
        for s0 in range(t * TI, min((t + 1) * TI, N), 16):
            if not bool(d[s0:min(s0 + 16, N)].any()):
                return "no dense-only row among ids %d..%d" % (s0 + 1, min(s0 + 16, N))
    return None
