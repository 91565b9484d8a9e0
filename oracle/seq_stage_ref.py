"""Stage-wise float64 reference of the SASRec session stack (forward and backward), with the measure its rounding error follows.
Test infrastructure: torch on the CPU only.

The stack exists in four forms (per-op f32, per-op x3, one launch per session, packed tiles) that must give the same mathematics.
Every STAGE of it (embed, ln1, qkv, attn, ln2, ffn1, ffn2, lnf; lnf_bwd, ffn_bwd, attn_bwd, qkv_bwd, wgrad, pos_grad) is restated
here as a function of that stage's own inputs, in ONE session-indexed layout ("canonical": [B, T, ..] for the K / V side and for an
unpruned block, [B, 1, ..] = position T-1 for the query / FFN side of a pruned last block, probabilities [B, heads, query, key]).
  run_stages(Arith("f64"), cfg, prm, cap)   every stage in float64 from the captured tensors `cap`, and beside every output its TERM
                                            SUM: the same expression with every term replaced by its absolute value (std, softmax
                                            probabilities and mean: their natural scale -- the value, 1, sum|x|/H).
  run_stages(emulation_arith(form, ..), ..) the kernels' STATED arithmetic in float32: for the x3 forms every product is bf16 hi/lo
                                            splits, lo.hi + hi.lo + hi.hi accumulated in float32 (x3_step_ref._x3mm), float32 row math,
                                            the reciprocal 1/sd multiplied in the LayerNorm backward, 1/sqrt(dh) multiplied in the x3
                                            attention, the bias gradient as the ones column of the x3 weight-gradient product; plain
                                            float32 for the per-op f32 form.
  check_stage(dev, ref, emu, ..)            each output within max(FACTOR x emulated error on the same inputs, FLOOR), measured row by row
                                            as max_c |x - ref| / (term_sum_row + 2^-24 max_rows term_sum) (weight gradients: entry by
                                            entry).  FACTOR and FLOOR are x3_step_ref's.
  chain(cfg, prm, ..)                       the float64 stages chained from the parameters: a complete capture (the host tests hold it
                                            to oracle/ader_ref_cpu.py, and plant faults into it).
  rows_to_canonical / p_to_canonical        one adapter per device layout (and their inverses, for the round-trip tests).
The cases of tests/test_gpu_seq_stage.py are built here too (CASES / make_batch), so that the host tests assert their conditions on
the very inputs the GPU runs."""
import numpy as np
import torch

from . import ader_ref_cpu as R
from .x3_step_ref import FACTOR, FLOOR, U24, ParityError, _split

f64, f32 = torch.float64, torch.float32


# =============================================================================================== arithmetic
class Arith:
    """kind: 'f64' (reference), 'f32' (plain float32), 'x3' (bf16 hi/lo splits).  attn: arithmetic of the attention products (the
    per-op x3 form with an odd head width runs the f32 attention core under x3 GEMMs).  fault: planted faults (host tests)."""

    def __init__(self, kind, attn=None, fault=None, last_fwd=None, last_bwd=None):
        self.kind, self.attn, self.fault = kind, attn or kind, fault or {}
        # the attention core of a pruned last block (one query row): its own kernels, forward and backward
        self.last_fwd, self.last_bwd = last_fwd or self.attn, last_bwd or self.attn
        self.dt = f64 if kind == "f64" else f32
        self.emu = kind != "f64"

    def t(self, x):
        return torch.as_tensor(x).to(self.dt)

    @staticmethod
    def _x3(A, B, drop_lohi=False):
        ah, al = _split(A)
        bh, bl = _split(B)
        if drop_lohi:
            return ah @ bl + ah @ bh
        return (al @ bh + ah @ bl) + ah @ bh

    def mm(self, A, W, name=None):
        if self.kind == "x3":
            f = self.fault.get("drop_lohi")                 # planted: the GEMM's name, or (name, session): only that session's rows
            if name is not None and f == name:
                return self._x3(A, W, drop_lohi=True)
            out = self._x3(A, W)
            if name is not None and isinstance(f, tuple) and f[0] == name:
                out = out.clone()
                out[f[1]] = self._x3(A[f[1]], W, drop_lohi=True)
            return out
        return A @ W

    def attn_kind(self, pruned, bwd=False):
        return (self.last_bwd if bwd else self.last_fwd) if pruned else self.attn

    def amm(self, A, B, kind):
        return self._x3(A, B) if kind == "x3" else A @ B


def emulation_arith(form, H, heads, fault=None):
    """The stated arithmetic of a form.  The one-row attention kernels of a pruned block (ader_attn_last_fwd / _bwd, ader_attnp_last_bwd:
    attn.hip, seqp_bwd.hip) are plain float32 fmaf cores in every form; only the one-launch and packed FORWARD keep the bf16x3 products
    for that row (it is a row of their tile)."""
    if form == "perop_f32":
        return Arith("f32", fault=fault)
    if form == "perop_x3":
        return Arith("x3", attn="x3" if (H // heads) % 2 == 0 else "f32", fault=fault, last_fwd="f32", last_bwd="f32")
    return Arith("x3", fault=fault, last_fwd="x3", last_bwd="f32")


def emulate_stage(form, cfg, prm, cap, fault=None):
    """Every stage of a capture in the form's stated float32 arithmetic: {(stage, block): (outputs, term sums)}."""
    return run_stages(emulation_arith(form, cfg["H"], cfg["heads"], fault=fault), cfg, prm, cap)


def _consts(ar, cfg):
    H, heads, rate = cfg["H"], cfg["heads"], cfg["rate"]
    sqrtH = float(np.float32(H ** 0.5)) if ar.emu else H ** 0.5
    sqrt_dh = float(np.float32((H // heads) ** 0.5))                         # (the oracle rounds this one to float32 too)
    if "dh_from_H" in ar.fault:
        sqrt_dh = float(np.float32(H ** 0.5))
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(rate))) if rate > 0 else 1.0
    return sqrtH, sqrt_dh, scale


def keep_mask(cfg, site, shape, fault=None):
    """Keep decisions [B, *shape] of a dropout site: oracle.dropout_keep per session from its GLOBAL row (cfg['grow'])."""
    B = cfg["B"]
    if cfg["rate"] == 0.0:
        return torch.ones((B,) + tuple(shape), dtype=torch.bool)
    per = int(np.prod(shape))
    grow = cfg["grow"]
    if fault and "wrong_split_base" in fault and cfg.get("split") is not None:
        grow = np.where(np.arange(B) >= cfg["split"], cfg["row0"] + np.arange(B), grow)
    out = np.stack([R.dropout_keep(per, int(grow[b]) * per, cfg["seed"], cfg["step"], site, cfg["rate"]) for b in range(B)])
    return torch.from_numpy(out.reshape((B,) + tuple(shape)))


def make_cfg(seq, T, H, L, heads, rate, seed, step, row0=0, split=None, row0_ex=0, prune_last=True):
    seq = np.asarray(seq)
    B = seq.shape[0]
    grow = np.arange(B) + row0
    if split is not None:
        grow = np.where(np.arange(B) >= split, np.arange(B) - split + row0_ex, grow)
    return dict(seq=torch.from_numpy(seq.astype(np.int64)), B=B, T=T, H=H, L=L, heads=heads, rate=float(rate), seed=seed, step=step,
                grow=grow, row0=row0, split=split, row0_ex=row0_ex, prune_last=prune_last, real=torch.from_numpy(seq != 0))


def qpos_of(cfg, l):
    T = cfg["T"]
    return [T - 1] if (cfg["prune_last"] and l == cfg["L"] - 1) else list(range(T))


# =============================================================================================== row math
def _rowmax(s):
    return s.max(-1).values


def _ln(ar, x, g, b, fault=None):
    H = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / H
    d = x - mean
    var = (d * d).sum(-1, keepdim=True) / (H - 1 if fault == "unbiased" else H)
    sd = (var + R.LN_EPS) ** 0.5
    y = g * (d / sd) + b
    s_y = g.abs() * ((x.abs() + mean.abs()) / sd) + b.abs()
    return y, mean[..., 0], sd[..., 0], _rowmax(s_y), x.abs().sum(-1) / H


def _ln_bwd(ar, dy, ady, x, mean, sd, g):
    """dx = (dxh - mean(dxh) - xh mean(dxh xh)) / sd; per-row gamma / beta terms dy*xh, dy.  ady: the term sum of dy."""
    H = x.shape[-1]
    mean, sd = mean.unsqueeze(-1), sd.unsqueeze(-1)
    rsd = 1.0 / sd
    xh = (x - mean) * rsd if ar.emu else (x - mean) / sd      # ln_bwd_rows / ln_bwd_rows_pk: one reciprocal per row, multiplied
    dxh = dy * g
    s1 = dxh.sum(-1, keepdim=True) / H
    s2 = (dxh * xh).sum(-1, keepdim=True) / H
    dx = (dxh - s1 - xh * s2) * rsd
    adxh = ady * g.abs()
    s_dx = (adxh + adxh.sum(-1, keepdim=True) / H + xh.abs() * ((adxh * xh.abs()).sum(-1, keepdim=True) / H)) * rsd
    return dx, _rowmax(s_dx), dy * xh, ady * xh.abs()


def _heads(x, heads):
    B, T, H = x.shape
    return x.view(B, T, heads, H // heads).permute(0, 2, 1, 3)


def _unheads(x):
    B, h, T, dh = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, T, h * dh)


def _w(ar, prm, l, name):
    return ar.t(prm["b%d.%s" % (l, name)])


# =============================================================================================== forward stages
def st_embed(ar, cfg, prm):
    sqrtH, _, scale = _consts(ar, cfg)
    seq, T, H = cfg["seq"], cfg["T"], cfg["H"]
    E, pos = ar.t(prm["emb"]), ar.t(prm["pos"])[:T]
    mask = (seq != 0).to(ar.dt).unsqueeze(-1)
    keep = keep_mask(cfg, R.SITE_EMB, (T, H), ar.fault).to(ar.dt)
    x = E[seq] * sqrtH + pos
    x0 = ((x * scale) * keep) * mask
    s = ((E[seq].abs() * sqrtH + pos.abs()) * scale) * mask
    return {"x0": x0}, {"x0": _rowmax(s)}


def st_ln1(ar, cfg, prm, l, x, xq):
    """x [B,T,H] block input (key mask), xq = its rows at the query positions."""
    fault = "unbiased" if ar.fault.get("unbiased_ln") == "ln1_%d" % l else None
    q_in, mean, sd, s_q, s_m = _ln(ar, xq, _w(ar, prm, l, "ln1_g"), _w(ar, prm, l, "ln1_b"), fault)
    kmask = torch.sign(x.sum(-1).abs())
    qmask = torch.sign(q_in.sum(-1).abs())
    return ({"q_in": q_in, "mean1": mean, "std1": sd, "kmask": kmask, "qmask": qmask},
            {"q_in": s_q, "mean1": s_m, "std1": sd.abs()})


def st_qkv(ar, cfg, prm, l, x, q_in):
    out, sc = {}, {}
    for nm, A, w, b in (("Q", q_in, "wq", "bq"), ("K", x, "wk", "bk"), ("V", x, "wv", "bv")):
        W, bias = _w(ar, prm, l, w), _w(ar, prm, l, b)
        out[nm] = ar.mm(A, W, "%s_%d" % (w, l)) + bias
        sc[nm] = _rowmax(A.abs() @ W.abs() + bias.abs())
    return out, sc


def _attn_masks(cfg, l, kmask, qpos, fault=None):
    T = cfg["T"]
    qp = torch.tensor(qpos)
    causal = torch.arange(T)[None, :] > qp[:, None]                        # [Tq,T] key after the query
    dead = (kmask == 0)[:, None, None, :] | causal[None, None]
    off = (fault or {}).get("causal_off")                                  # planted: (block, session, query) reads one key too many
    if off is not None and off[0] == l and off[2] in qpos and off[2] + 1 < T:
        dead[off[1], :, qpos.index(off[2]), off[2] + 1] = False
    return dead


def st_attn(ar, cfg, prm, l, Q, K, V, q_in, kmask, qmask, qpos):
    _, sqrt_dh, scale = _consts(ar, cfg)
    heads, T = cfg["heads"], cfg["T"]
    Qh, Kh, Vh = _heads(Q, heads), _heads(K, heads), _heads(V, heads)
    kind = ar.attn_kind(len(qpos) == 1 and T > 1)
    s = ar.amm(Qh, Kh.transpose(-1, -2), kind)
    s = s * (1.0 / np.float32(sqrt_dh)).item() if (ar.emu and kind == "x3") else s / sqrt_dh
    s = torch.where(_attn_masks(cfg, l, kmask, qpos, ar.fault), torch.full_like(s, R.NEG_PAD), s)
    P = torch.softmax(s, -1)
    leak = ar.fault.get("tile_leak")            # planted: (block, session, other session) -- the other session's last row is a key too
    xtra = None
    if leak is not None and leak[0] == l:
        b, b2 = leak[1], leak[2]
        sx = (Qh[b] @ Kh[b2, :, T - 1, :].unsqueeze(-1)) / sqrt_dh
        Pb = torch.softmax(torch.cat([s[b], sx], -1), -1)
        if len(leak) > 3:                        # ... for one query only
            only = torch.zeros(len(qpos), dtype=torch.bool)
            only[qpos.index(leak[3])] = True
            Pb = torch.where(only[None, :, None], Pb, torch.cat([P[b], torch.zeros_like(sx)], -1))
        P = P.clone()
        P[b] = Pb[..., :T]
        xtra = (b, (Pb[..., T:] * qmask[b, None, :, None]) * scale * Vh[b2, :, T - 1, :].unsqueeze(1))
    keep = keep_mask(cfg, R.site_attn(l), (heads, T, T), ar.fault)[:, :, qpos, :].to(ar.dt)
    a = ((P * qmask[:, None, :, None]) * scale) * keep
    o = ar.amm(a, Vh, kind)
    if xtra is not None:
        o = o.clone()
        o[xtra[0]] = o[xtra[0]] + xtra[1]
    o = _unheads(o)
    x1 = o + q_in
    s_x1 = _unheads(a.abs() @ Vh.abs()) + q_in.abs()
    return {"P": P, "x1": x1}, {"P": torch.ones(P.shape[0], P.shape[2], dtype=ar.dt), "x1": _rowmax(s_x1)}


def p_rows(P):
    """[B,heads,Tq,T] -> [B,Tq,heads*T]: the probabilities of a (session, query) as one row of the measure."""
    B, h, Tq, T = P.shape
    return P.permute(0, 2, 1, 3).reshape(B, Tq, h * T)


def st_ln2(ar, cfg, prm, l, x1):
    fault = "unbiased" if ar.fault.get("unbiased_ln") == "ln2_%d" % l else None
    y, mean, sd, s_y, s_m = _ln(ar, x1, _w(ar, prm, l, "ln2_g"), _w(ar, prm, l, "ln2_b"), fault)
    return {"y": y, "mean2": mean, "std2": sd}, {"y": s_y, "mean2": s_m, "std2": sd.abs()}


def st_ffn1(ar, cfg, prm, l, y, qpos):
    _, _, scale = _consts(ar, cfg)
    W, b = _w(ar, prm, l, "w1"), _w(ar, prm, l, "b1")
    keep = keep_mask(cfg, R.site_ffn1(l), (cfg["T"], cfg["H"]), ar.fault)[:, qpos].to(ar.dt)
    h = (torch.relu(ar.mm(y, W, "w1_%d" % l) + b) * scale) * keep
    return {"h1d": h}, {"h1d": _rowmax((y.abs() @ W.abs() + b.abs()) * scale)}


def st_ffn2(ar, cfg, prm, l, h1d, y, qpos):
    _, _, scale = _consts(ar, cfg)
    W, b = _w(ar, prm, l, "w2"), _w(ar, prm, l, "b2")
    keep = keep_mask(cfg, R.site_ffn2(l), (cfg["T"], cfg["H"]), ar.fault)[:, qpos].to(ar.dt)
    mask = cfg["real"][:, qpos].to(ar.dt).unsqueeze(-1)
    res = y * 0 if ar.fault.get("no_residual") == l else y
    x2 = (((ar.mm(h1d, W, "w2_%d" % l) + b) * scale) * keep + res) * mask
    s = ((h1d.abs() @ W.abs() + b.abs()) * scale + y.abs()) * mask
    return {"x2": x2}, {"x2": _rowmax(s)}


def st_lnf(ar, cfg, prm, xlast):
    fault = "unbiased" if ar.fault.get("unbiased_ln") == "lnf" else None
    rep, mean, sd, s_y, s_m = _ln(ar, xlast, ar.t(prm["lnf_g"]), ar.t(prm["lnf_b"]), fault)
    return {"rep": rep, "meanf": mean, "stdf": sd}, {"rep": s_y, "meanf": s_m, "stdf": sd.abs()}


# =============================================================================================== backward stages
def _colsum(rows, arows, valid):
    v = valid.unsqueeze(-1)             # (where, not a product: a row that does not exist may hold sd = 0, hence NaN terms)
    H, z = rows.shape[-1], torch.zeros((), dtype=rows.dtype)
    return torch.where(v, rows, z).reshape(-1, H).sum(0), torch.where(v, arows, z).reshape(-1, H).sum(0)


def st_lnf_bwd(ar, cfg, prm, drep, xlast, meanf, stdf):
    dx, s_dx, gr, agr = _ln_bwd(ar, drep, drep.abs(), xlast, meanf, stdf, ar.t(prm["lnf_g"]))
    every = torch.ones(drep.shape[0], dtype=torch.bool)                 # (an all-padding session has rep = beta: its drep reaches beta, and gamma with xh = 0)
    dg, s_dg = _colsum(gr, agr, every)
    db, s_db = _colsum(drep, drep.abs(), every)
    return {"dxL": dx, "lnf_g": dg, "lnf_b": db}, {"dxL": s_dx, "lnf_g": s_dg, "lnf_b": s_db}


def st_ffn_bwd(ar, cfg, prm, l, dx2, h1d, x1, mean2, std2, qpos):
    _, _, scale = _consts(ar, cfg)
    valid = cfg["real"][:, qpos]
    mask = valid.to(ar.dt).unsqueeze(-1)
    keep2 = keep_mask(cfg, R.site_ffn2(l), (cfg["T"], cfg["H"]), ar.fault)[:, qpos].to(ar.dt)
    W2, W1 = _w(ar, prm, l, "w2"), _w(ar, prm, l, "w1")
    g = dx2 * mask
    dh2 = (g * scale) * keep2
    alive = (h1d != 0).to(ar.dt)                                          # the device's own ReLU / dropout decision
    da = (ar.mm(dh2, W2.t(), "w2t_%d" % l) * scale) * alive
    s_da = ((dh2.abs() @ W2.abs().t()) * scale) * alive
    dy = ar.mm(da, W1.t(), "w1t_%d" % l) + g
    ady = da.abs() @ W1.abs().t() + g.abs()
    dx1, s_dx1, gr, agr = _ln_bwd(ar, dy, ady, x1, mean2, std2, _w(ar, prm, l, "ln2_g"))
    dg, s_dg = _colsum(gr, agr, valid)
    db, s_db = _colsum(dy, ady, valid)
    return ({"dh2": dh2, "da": da, "dx1": dx1, "ln2_g": dg, "ln2_b": db},
            {"dh2": _rowmax(g.abs() * scale), "da": _rowmax(s_da), "dx1": s_dx1, "ln2_g": s_dg, "ln2_b": s_db})


def st_attn_bwd(ar, cfg, prm, l, dx1, Q, K, V, P, qmask, qpos):
    _, sqrt_dh, scale = _consts(ar, cfg)
    heads, T = cfg["heads"], cfg["T"]
    Qh, Kh, Vh, dO = _heads(Q, heads), _heads(K, heads), _heads(V, heads), _heads(dx1, heads)
    keep = keep_mask(cfg, R.site_attn(l), (heads, T, T), ar.fault)[:, :, qpos, :].to(ar.dt)
    m = (qmask[:, None, :, None] * scale) * keep
    Pd = P * m
    kind = ar.attn_kind(len(qpos) == 1 and T > 1, bwd=True)
    dV = ar.amm(Pd.transpose(-1, -2), dO, kind)
    dP = ar.amm(dO, Vh.transpose(-1, -2), kind) * m
    adP = (dO.abs() @ Vh.abs().transpose(-1, -2)) * m
    dS = P * (dP - (dP * P).sum(-1, keepdim=True))
    adS = P * (adP + (adP * P).sum(-1, keepdim=True))
    dQ = ar.amm(dS, Kh, kind) / sqrt_dh
    dK = ar.amm(dS.transpose(-1, -2), Qh, kind) / sqrt_dh
    return ({"dQ": _unheads(dQ), "dK": _unheads(dK), "dV": _unheads(dV)},
            {"dQ": _rowmax(_unheads(adS @ Kh.abs() / sqrt_dh)), "dK": _rowmax(_unheads(adS.transpose(-1, -2) @ Qh.abs() / sqrt_dh)),
             "dV": _rowmax(_unheads(Pd.abs().transpose(-1, -2) @ dO.abs()))})


def st_qkv_bwd(ar, cfg, prm, l, dQ, dx1, dK, dV, x, mean1, std1, qpos):
    _, _, scale = _consts(ar, cfg)
    Wq, Wk, Wv = _w(ar, prm, l, "wq"), _w(ar, prm, l, "wk"), _w(ar, prm, l, "wv")
    valid = cfg["real"][:, qpos]
    dqin = ar.mm(dQ, Wq.t(), "wqt_%d" % l) + dx1
    adqin = dQ.abs() @ Wq.abs().t() + dx1.abs()
    dxq, s_dxq, gr, agr = _ln_bwd(ar, dqin, adqin, x[:, qpos], mean1, std1, _w(ar, prm, l, "ln1_g"))
    dkv = ar.mm(dK, Wk.t(), "wkt_%d" % l) + ar.mm(dV, Wv.t(), "wvt_%d" % l)
    s = _rowmax(dK.abs() @ Wk.abs().t() + dV.abs() @ Wv.abs().t())
    dx = dkv.clone()
    dx[:, qpos] = dx[:, qpos] + dxq
    s = s.clone()
    s[:, qpos] = s[:, qpos] + s_dxq
    if l == 0:                                                            # the prologue: mask and dropout of the embedding rows
        keep = keep_mask(cfg, R.SITE_EMB, (cfg["T"], cfg["H"]), ar.fault).to(ar.dt)
        dx = ((dx * cfg["real"].to(ar.dt).unsqueeze(-1)) * scale) * keep
        s = s * scale
    dg, s_dg = _colsum(gr, agr, valid)
    db, s_db = _colsum(dqin, adqin, valid)
    return {"dxi": dx, "ln1_g": dg, "ln1_b": db}, {"dxi": s, "ln1_g": s_dg, "ln1_b": s_db}


def st_wgrad(ar, A, G, valid, name=None, stale=None):
    """dW = A^T G, db = colsum(G) over the real rows.  stale: (A row, G row) of one row that is NOT real, included all the same."""
    v, z = valid.unsqueeze(-1), torch.zeros((), dtype=A.dtype)
    H = A.shape[-1]
    A2, G2 = torch.where(v, A, z).reshape(-1, H), torch.where(v, G, z).reshape(-1, H)
    if stale is not None:
        A2, G2 = torch.cat([A2, stale[0].reshape(1, H).to(A2.dtype)]), torch.cat([G2, stale[1].reshape(1, H).to(A2.dtype)])
    dW = ar.mm(A2.t().contiguous(), G2, name)
    s_W = A2.abs().t() @ G2.abs()
    # gemm_x3.hip: the bias gradient is the ones column of the augmented A, through the same x3 product: sum(G_hi + G_lo)
    db = ar.mm(torch.ones(1, A2.shape[0], dtype=A2.dtype), G2)[0] if ar.kind == "x3" else G2.sum(0)
    return {"dW": dW, "db": db}, {"dW": s_W, "db": G2.abs().sum(0)}


def st_pos_grad(ar, cfg, dx0):
    d = torch.where(cfg["real"].unsqueeze(-1), dx0, torch.zeros((), dtype=dx0.dtype))
    return {"pos": d.sum(0)}, {"pos": d.abs().sum(0)}


# =============================================================================================== all stages of a capture
def run_stages(ar, cfg, prm, cap):
    """Every stage from the captured tensors `cap` (canonical layout; see chain for its keys).  Returns {(stage, block): (outputs,
    term sums)}; the output names are the capture's names."""
    L, T = cfg["L"], cfg["T"]
    c = lambda k: ar.t(cap[k])      # noqa: E731
    res = {("embed", 0): st_embed(ar, cfg, prm)}
    for l in range(L):
        qp = qpos_of(cfg, l)
        k = lambda s: "%s%d" % (s, l)      # noqa: E731
        x = c(k("x"))
        xq = x[:, [T - 2]] if (ar.fault.get("prune_T2") and len(qp) == 1) else x[:, qp]
        res[("ln1", l)] = st_ln1(ar, cfg, prm, l, x, xq)
        res[("qkv", l)] = st_qkv(ar, cfg, prm, l, x, c(k("q_in")))
        res[("attn", l)] = st_attn(ar, cfg, prm, l, c(k("Q")), c(k("K")), c(k("V")), c(k("q_in")), c(k("kmask")), c(k("qmask")), qp)
        res[("ln2", l)] = st_ln2(ar, cfg, prm, l, c(k("x1")))
        res[("ffn1", l)] = st_ffn1(ar, cfg, prm, l, c(k("y")), qp)
        res[("ffn2", l)] = st_ffn2(ar, cfg, prm, l, c(k("h1d")), c(k("y")), qp)
    xlast = c("x%d" % L)[:, -1]
    res[("lnf", 0)] = st_lnf(ar, cfg, prm, xlast)
    if "drep" not in cap:
        return res
    res[("lnf_bwd", 0)] = st_lnf_bwd(ar, cfg, prm, c("drep"), xlast, c("meanf"), c("stdf"))
    for l in reversed(range(L)):
        qp = qpos_of(cfg, l)
        k = lambda s: "%s%d" % (s, l)      # noqa: E731
        valid = cfg["real"][:, qp]
        res[("ffn_bwd", l)] = st_ffn_bwd(ar, cfg, prm, l, c(k("dxo")), c(k("h1d")), c(k("x1")), c(k("mean2")), c(k("std2")), qp)
        res[("attn_bwd", l)] = st_attn_bwd(ar, cfg, prm, l, c(k("dx1")), c(k("Q")), c(k("K")), c(k("V")), c(k("P")), c(k("qmask")), qp)
        res[("qkv_bwd", l)] = st_qkv_bwd(ar, cfg, prm, l, c(k("dQ")), c(k("dx1")), c(k("dK")), c(k("dV")), c(k("x")), c(k("mean1")),
                                         c(k("std1")), qp)
        out, sc = {}, {}
        stale = cap.get("_stale")
        for w, b, A, G, vd in (("w2", "b2", k("h1d"), k("dh2"), valid), ("w1", "b1", k("y"), k("da"), valid),
                               ("wq", "bq", k("q_in"), k("dQ"), valid), ("wk", "bk", k("x"), k("dK"), cfg["real"]),
                               ("wv", "bv", k("x"), k("dV"), cfg["real"])):
            st = stale[1:] if (stale is not None and stale[0] == "%s_%d" % (w, l)) else None
            o, s = st_wgrad(ar, c(A), c(G), vd, "d%s_%d" % (w, l), stale=st)
            out[w], out[b], sc[w], sc[b] = o["dW"], o["db"], s["dW"], s["db"]
        res[("wgrad", l)] = (out, sc)
    res[("pos_grad", 0)] = st_pos_grad(ar, cfg, c("dxi0"))
    return res


# names a stage's outputs carry in the capture (block-indexed names get the block number appended)
FWD_STAGES = ("embed", "ln1", "qkv", "attn", "ln2", "ffn1", "ffn2", "lnf")
BWD_STAGES = ("lnf_bwd", "ffn_bwd", "attn_bwd", "qkv_bwd", "wgrad", "pos_grad")
GRAD_OUTPUTS = {"lnf_bwd": ("lnf_g", "lnf_b"), "ffn_bwd": ("ln2_g", "ln2_b"), "qkv_bwd": ("ln1_g", "ln1_b"),
                "wgrad": ("wq", "bq", "wk", "bk", "wv", "bv", "w1", "b1", "w2", "b2"), "pos_grad": ("pos",)}


def cap_name(stage, l, name, L):
    """The capture key of output `name` of (stage, block l); parameter gradients live under 'g:<parameter>'."""
    if name in GRAD_OUTPUTS.get(stage, ()):
        return "g:" + (name if stage in ("lnf_bwd", "pos_grad") else "b%d.%s" % (l, name))
    if stage == "embed":
        return "x0"
    if stage in ("lnf", "lnf_bwd"):
        return {"dxL": "dxo%d" % (L - 1)}.get(name, name)
    if name == "x2":
        return "x%d" % (l + 1)
    if name == "dxi" and l > 0:
        return "dxo%d" % (l - 1)
    return "%s%d" % (name, l)


def chain(cfg, prm, drep_fn=None, ar=None):
    """The float64 stages chained from the parameters: a complete capture.  drep_fn(rep) -> drep [B,H]."""
    ar = ar or Arith("f64")
    L, T = cfg["L"], cfg["T"]
    cap = {}
    x = st_embed(ar, cfg, prm)[0]["x0"]
    cap["x0"] = x
    for l in range(L):
        qp = qpos_of(cfg, l)
        o = st_ln1(ar, cfg, prm, l, x, x[:, qp])[0]
        o.update(st_qkv(ar, cfg, prm, l, x, o["q_in"])[0])
        o.update(st_attn(ar, cfg, prm, l, o["Q"], o["K"], o["V"], o["q_in"], o["kmask"], o["qmask"], qp)[0])
        o.update(st_ln2(ar, cfg, prm, l, o["x1"])[0])
        o.update(st_ffn1(ar, cfg, prm, l, o["y"], qp)[0])
        x = st_ffn2(ar, cfg, prm, l, o["h1d"], o["y"], qp)[0]["x2"]
        for k_, v in o.items():
            cap["%s%d" % (k_, l)] = v
        cap["x%d" % (l + 1)] = x
    o = st_lnf(ar, cfg, prm, x[:, -1])[0]
    cap.update(o)
    if drep_fn is None:
        return cap
    cap["drep"] = ar.t(drep_fn(cap["rep"]))
    o = st_lnf_bwd(ar, cfg, prm, cap["drep"], x[:, -1], cap["meanf"], cap["stdf"])[0]
    cap["g:lnf_g"], cap["g:lnf_b"] = o["lnf_g"], o["lnf_b"]
    dxo = o["dxL"].unsqueeze(1)
    if not cfg["prune_last"]:
        full = torch.zeros(cfg["B"], T, cfg["H"], dtype=ar.dt)
        full[:, -1] = o["dxL"]
        dxo = full
    for l in reversed(range(L)):
        qp = qpos_of(cfg, l)
        k = lambda s: cap["%s%d" % (s, l)]      # noqa: E731
        cap["dxo%d" % l] = dxo
        o = st_ffn_bwd(ar, cfg, prm, l, dxo, k("h1d"), k("x1"), k("mean2"), k("std2"), qp)[0]
        o.update(st_attn_bwd(ar, cfg, prm, l, o["dx1"], k("Q"), k("K"), k("V"), k("P"), k("qmask"), qp)[0])
        o.update(st_qkv_bwd(ar, cfg, prm, l, o["dQ"], o["dx1"], o["dK"], o["dV"], k("x"), k("mean1"), k("std1"), qp)[0])
        for nm in ("dh2", "da", "dx1", "dQ", "dK", "dV"):
            cap["%s%d" % (nm, l)] = o[nm]
        for nm in ("ln1_g", "ln1_b", "ln2_g", "ln2_b"):
            cap["g:b%d.%s" % (l, nm)] = o[nm]
        dxo = o["dxi"]
        if l == 0:
            cap["dxi0"] = dxo
    res = run_stages(ar, cfg, prm, cap)
    for l in range(L):
        for nm, v in res[("wgrad", l)][0].items():
            cap["g:b%d.%s" % (l, nm)] = v
    cap["g:pos"] = res[("pos_grad", 0)][0]["pos"]
    return cap


# =============================================================================================== check
def _valid_of(cfg, stage, l, name):
    """Rows of output `name` that are judged: real positions (query positions of the block), non-empty sessions for [B, ..] tensors;
    parameter gradients: every entry."""
    if name in GRAD_OUTPUTS.get(stage, ()):
        return None
    if stage in ("lnf", "lnf_bwd"):
        return cfg["real"][:, cfg["T"] - 1]
    if stage == "embed" or name in ("K", "V", "kmask", "dK", "dV", "dxi"):
        return cfg["real"]
    return cfg["real"][:, qpos_of(cfg, l)]


def stage_errors(x, ref, scale, valid, entrywise):
    x, ref, scale = torch.as_tensor(x).to(f64), ref.to(f64), scale.to(f64)
    d = (x - ref).abs()
    if not entrywise and d.dim() > scale.dim():
        d = d.max(-1).values
    if valid is not None:
        scale = torch.where(valid, scale, torch.zeros_like(scale))
        d = torch.where(valid, d, torch.zeros_like(d))
    smax = float(scale.max()) if scale.numel() else 0.0
    return d / (scale + U24 * smax + 1e-300)


def check_stage(dev, ref, emu, cfg, stage, l, form="", exact=("kmask", "qmask")):
    """dev / emu: {name: tensor} outputs of (stage, block l) in the canonical layout; ref: (outputs, term sums) of run_stages.
    Returns {name: (error, emulated error, bound, worst index)}; raises ParityError naming form, stage, block and the worst
    (session, position) when an error exceeds max(FACTOR x emulated error, FLOOR).  (kmask / qmask are exact: judged by the tests.)"""
    out, bad = stage_report(dev, ref, emu, cfg, stage, l, form, exact)
    if bad:
        raise ParityError("; ".join(bad))
    return out


def stage_report(dev, ref, emu, cfg, stage, l, form="", exact=("kmask", "qmask")):
    """check_stage without the raise: ({name: (error, emulated error, bound, worst index)}, [complaints])."""
    out, bad = {}, []
    rout, rsc = ref
    for name, r in rout.items():
        if name in exact:
            continue
        if name not in dev:                                   # (a renamed buffer must not drop a check silently)
            bad.append("%s %s block %d %s: not captured" % (form, stage, l, name))
            continue
        x, e = dev[name], emu[name]
        if name == "P":
            x, e, r = p_rows(torch.as_tensor(x)), p_rows(e), p_rows(r)
        entry = name in GRAD_OUTPUTS.get(stage, ())
        valid = _valid_of(cfg, stage, l, name)
        e_dev = stage_errors(x, r, rsc[name], valid, entry)
        e_emu = stage_errors(e, r, rsc[name], valid, entry)
        err, base = float(e_dev.max()), float(e_emu.max())
        bound = max(FACTOR * base, FLOOR)
        worst = tuple(int(i) for i in np.unravel_index(int(torch.argmax(e_dev)), e_dev.shape)) if e_dev.numel() else ()
        out[name] = (err, base, bound, worst)
        if not err <= bound:
            if entry or not worst:
                where = "entry %s" % (worst,)
            else:
                qp = qpos_of(cfg, l)
                t = worst[1] if (len(worst) > 1 and e_dev.shape[1] == cfg["T"]) else (qp[worst[1]] if len(worst) > 1 else cfg["T"] - 1)
                where = "session %d, position %d" % (worst[0], t)
            bad.append("%s %s block %d %s: %.3g > bound %.3g (emulated %.3g); worst %s" % (form, stage, l, name, err, bound, base, where))
    return out, bad


def dev_outputs(cap, stage, l, L, names):
    """The captured (device) tensors of a stage's outputs, under the stage's own output names."""
    out = {}
    for nm in names:
        key = cap_name(stage, l, nm, L)
        if key in cap:
            t = cap[key]
            if stage == "lnf_bwd" and nm == "dxL" and t.dim() == 3:
                t = t[:, -1]
            out[nm] = t
    return out


def check_capture(cap, cfg, prm, form, emu_arith=None, raise_=True, forward_only=False):
    """check_stage on every stage of a capture.  Returns [(stage, block, name, error, emulated error, bound, worst)] (raise_=False:
    and the complaints, instead of raising them).  forward_only: the capture of a forward(save=True) -- it holds no backward tensor,
    and only the stages embed .. lnf (FWD_STAGES) are restated and judged, in the same measure and bound."""
    if forward_only:
        cap = {k: v for k, v in cap.items() if k != "drep"}          # (run_stages stops behind lnf without it)
    ref = run_stages(Arith("f64"), cfg, prm, cap)
    assert not forward_only or {st for st, _ in ref} == set(FWD_STAGES)
    emu = run_stages(emu_arith, cfg, prm, cap) if emu_arith is not None else emulate_stage(form, cfg, prm, cap)
    rows, bad = [], []
    for (stage, l), r in ref.items():
        dev = dev_outputs(cap, stage, l, cfg["L"], r[0].keys())
        res, b = stage_report(dev, r, emu[(stage, l)][0], cfg, stage, l, form)
        bad += b
        rows += [(stage, l, nm) + v for nm, v in res.items()]
    if not raise_:
        return rows, bad, ref
    if bad:
        raise ParityError("\n".join(bad))
    return rows


def format_rows(rows, label):
    """One line per stage: device error / emulated error of its worst output, and the worst row."""
    by = {}
    for stage, l, nm, err, base, bound, worst in rows:
        key = (stage, l)
        ratio = err / max(base, FLOOR / FACTOR)
        if key not in by or ratio > by[key][0]:
            by[key] = (ratio, nm, err, base, worst)
    return ["seq-stage %s %s[%d]: %.2fx (%s err %.2e emu %.2e) worst %s" % (label, s, l, v[0], v[1], v[2], v[3], v[4])
            for (s, l), v in by.items()]


# =============================================================================================== layouts
def rows_to_canonical(t, layout, B, T, plan=None):
    """[B*T, ..] (layout 'rows'), tile order [tiles*64, ..] ('tiles': plan = dict srow0, slen) or compact [B, ..] ('compact')
    -> [B, T, ..] / [B, 1, ..]; absent positions are zeros."""
    t = torch.as_tensor(t)
    if layout == "compact":
        return t.reshape((B, 1) + tuple(t.shape[1:]))
    if layout == "rows":
        return t.reshape((B, T) + tuple(t.shape[1:]))
    out = torch.zeros((B, T) + tuple(t.shape[1:]), dtype=t.dtype)
    for b in range(B):
        n, p0 = int(plan["slen"][b]), int(plan["srow0"][b])
        out[b, T - n:] = t[p0:p0 + n]
    return out


def rows_from_canonical(c, layout, plan=None, n_tiles=None):
    B, T = c.shape[:2]
    if layout in ("compact", "rows"):
        return c.reshape((-1,) + tuple(c.shape[2:]))
    out = torch.zeros((n_tiles * 64,) + tuple(c.shape[2:]), dtype=c.dtype)
    for b in range(B):
        n, p0 = int(plan["slen"][b]), int(plan["srow0"][b])
        out[p0:p0 + n] = c[b, T - n:]
    return out


def p_to_canonical(P, layout, B, T, heads, plan=None):
    """Saved probabilities -> [B, heads, query, key].  'qk': [B,heads,query,key] (ader_attn_fwd); 'kq': [B,heads,key,query] (x3
    attention, one-launch form); 'tiles': [tile][key][query] over 64 tile rows; 'last': [B,heads,T] / [B,T] of query T-1."""
    P = torch.as_tensor(P).reshape(-1)
    if layout == "qk":
        return P[:B * heads * T * T].reshape(B, heads, T, T)
    if layout == "kq":
        return P[:B * heads * T * T].reshape(B, heads, T, T).transpose(-1, -2).contiguous()
    if layout == "last":
        return P[:B * heads * T].reshape(B, heads, 1, T)
    Pt = P.reshape(-1, 64, 64)
    out = torch.zeros(B, 1, T, T, dtype=P.dtype)
    for b in range(B):
        n, p0 = int(plan["slen"][b]), int(plan["srow0"][b])
        u, r0 = divmod(p0, 64)
        out[b, 0, T - n:, T - n:] = Pt[u, r0:r0 + n, r0:r0 + n].t()
    return out


def p_from_canonical(Pc, layout, plan=None, n_tiles=None):
    B, heads, Tq, T = Pc.shape
    if layout == "qk":
        return Pc.reshape(-1)
    if layout == "kq":
        return Pc.transpose(-1, -2).reshape(-1)
    if layout == "last":
        return Pc.reshape(-1)
    out = torch.zeros(n_tiles, 64, 64, dtype=Pc.dtype)
    for b in range(B):
        n, p0 = int(plan["slen"][b]), int(plan["srow0"][b])
        u, r0 = divmod(p0, 64)
        out[u, r0:r0 + n, r0:r0 + n] = Pc[b, 0, T - n:, T - n:].t()
    return out.reshape(-1)


# =============================================================================================== cases
MIXED40 = [1, 16, 17, 32, 33, 40, 41, -1, 0, 1, 1, 2, 3, 5, 8, 13, 16, 16, 16, 16, 4, 4, 4, 4, 7, 9, 11, 2, 1, 6, 15, 16, 16, 15, 14, 3, 2, 1,
           1, 10]                      # -1 = T; clipped to T
ITEM_NUM, MAX_ID = 700, 650
WINDOWS = ((17, 49, 224), (49, 49, 0))


def _case(name, T, H, L, heads, law, rate, forms, split=None, logits="f32", windows=(WINDOWS[0],)):
    return dict(name=name, T=T, H=H, L=L, heads=heads, law=law, rate=rate, forms=forms, split=split, logits=logits, windows=windows)


CASES = [
    _case("A", 64, 150, 2, (1,), "mixed40", 0.3, ("perop_f32", "fused", "packed"), split=dict(n_train=30, row0=120, row0_ex=1000),
          windows=WINDOWS),
    _case("B", 50, 150, 4, (1,), "mixed40", 0.3, ("fused", "packed")),
    _case("C", 33, 64, 2, (1, 2), "mixed40", 0.0, ("perop_f32", "perop_x3", "fused", "packed")),
    _case("D", 5, 10, 1, (1,), [5, 1, 2], 0.3, ("perop_f32", "fused", "packed")),
    _case("E", 64, 150, 1, (1,), [64], 0.3, ("fused", "packed")),
    _case("F", 50, 150, 2, (1,), "geom70", 0.3, ("packed",), logits="x3"),
    _case("G", 50, 150, 2, (3,), "uniform9", 0.3, ("perop_x3", "perop_f32")),
    _case("H", 50, 150, 2, (2,), "uniform9", 0.3, ("perop_x3",)),
    _case("I", 50, 158, 2, (1,), "uniform9", 0.3, ("perop_f32",)),
]
CASE_IDS = [c["name"] for c in CASES]


def runs_of(case):
    """(form, heads, window) of every engine run of a case: the per-op x3 form needs >= 2 heads (else the session kernels take
    over), the session kernels exactly one; the per-op f32 form runs at the case's first head count."""
    out = []
    for form in case["forms"]:
        if form == "perop_x3":
            hs = [h for h in case["heads"] if h >= 2]
        elif form == "perop_f32":
            hs = [case["heads"][0]]
        else:
            hs = [h for h in case["heads"] if h == 1]
        for h in hs:
            for w in (case["windows"] if form == "packed" else (None,)):
                out.append((form, h, w))
    return out


def lengths_of(case):
    T, law = case["T"], case["law"]
    if law == "mixed40":
        return np.array([T if v < 0 else min(v, T) for v in MIXED40])
    if law == "geom70":
        return np.clip(np.random.RandomState(70).geometric(0.2, size=70), 1, T)
    if law == "uniform9":
        return np.random.RandomState(9).randint(1, T + 1, size=9)
    return np.array(law)


def make_batch(case, seed=0):
    """dict seq [B,T] int32 (train rows first), pos [n_train], ex_pos [n_ex] or None, N."""
    rs = np.random.RandomState(500 + seed)
    ln = lengths_of(case)
    B, T = len(ln), case["T"]
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        if ln[b]:
            seq[b, T - ln[b]:] = rs.randint(1, MAX_ID + 1, size=ln[b])
    n_ex = B - case["split"]["n_train"] if case["split"] else 0
    pos = rs.randint(1, MAX_ID + 1, size=B - n_ex).astype(np.int32)
    ex_pos = rs.randint(1, MAX_ID + 1, size=n_ex).astype(np.int32) if n_ex else None
    return dict(seq=seq, pos=pos, ex_pos=ex_pos, N=MAX_ID, lambda_=0.6 if n_ex else 0.0)


def cfg_of(case, batch, heads, seed, step=4):
    sp = case["split"]
    return make_cfg(batch["seq"], case["T"], case["H"], case["L"], heads, case["rate"], seed, step, row0=sp["row0"] if sp else 0,
                    split=sp["n_train"] if sp else None, row0_ex=sp["row0_ex"] if sp else 0)
