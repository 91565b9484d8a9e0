"""Stage-wise float64 parity of the SASRec session stack, forward and backward, in its four forms: the per-op f32 kernels, the
per-op x3 kernels, one launch per session (ader_seq_fwd / ader_seq_bwd_*) and the packed tiles (ader_seqp_*).

One loss_and_grad call runs per case and form (no optimiser: nothing is deferred to a side stream).  The device's OWN inputs to
every stage are read back -- the saved activations of Engine._act, the backward tensors of the workspace under the names
_bwd_block_desc / _blocks_backward give them, the ping-pong block gradients cloned right behind the launch that wrote them -- brought
into one session-indexed layout, and only that stage is restated in float64 on the CPU (oracle/seq_stage_ref.py).  Every output is
judged ROW BY ROW in the term-sum measure of that module (weight gradients entry by entry) against max(8 x the error of a float32
emulation of the kernels' stated arithmetic on the same inputs, 16 float32 ulps): a wrong row of one session, a wrong small row or
a wrong entry of a weight gradient fed by a few positions cannot hide under the tensor's maximum, and a failure names form, stage,
block and (session, position).  Exact: the masks, the dropout zero pattern of x0 and h1d, rep of an all-padding session = beta of
the final LayerNorm, rows 0 and > N of the table gradient, the device plan = numpy_plan, and -- packed form -- every tile row at or
beyond its tile's row count and every saved probability outside its session's causal block bitwise zero.  Every run also asserts
which launchers ran (and which did not), and that every output of every stage was judged.

Cases (oracle/seq_stage_ref.CASES): the smallest shapes at which each mechanism engages; see the table there and
profiles/seq_stage_parity.txt for every case x form x stage.

Measured on an MI355X (device error / emulated error, worst over the 20 runs; profiles/seq_stage_parity.txt has every line):
    embed 1.00x   ln1 1.08x   qkv 1.02x   attn 2.03x (G per-op f32, x1)   ln2 1.26x   ffn1 1.02x   ffn2 1.01x   lnf 1.11x
    lnf_bwd 1.00x   ffn_bwd 1.11x   attn_bwd 1.43x (G per-op x3, dK)   qkv_bwd 1.08x   wgrad 1.60x (A per-op f32, wk)   pos_grad 1.02x
The bound is 8x: the unchanged kernels sit on the emulation in every form, and every exact check holds (no tile row beyond a tile's
row count is written; the device plan is numpy_plan).  The first run found the EMULATION short of a stated step: the x3 weight-
gradient product forms the bias gradient as the ones column of the augmented operand (gemm_x3.hip), i.e. sum(G_hi + G_lo) -- a plain
float32 column sum is 8 .. 58x more exact than that (device 1e-6 .. 7e-6 of sum|G|); emulated as stated, the ratio is 1.0x.
The one-row attention kernels of a pruned block (ader_attn_last_fwd / _bwd, ader_attnp_last_bwd) are float32 cores in every form and
are emulated as such (0.5 .. 2.0x); only the one-launch and packed forward keep the x3 products for that row (1.0x).

NOT covered here: the exact zero pattern of the attention term (the dropped probabilities are not stored; P and x1 are judged in
the measure, with the oracle's keep decisions as inputs, so a wrong decision is an order-one error of x1)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from stress_handoffs import numpy_plan  # noqa: E402
from test_gpu_parity import _engine  # noqa: E402

from oracle import seq_stage_ref as S  # noqa: E402

SEED, STEP = 3, 4
RUNS = [(c, f, h, w) for c in S.CASES for f, h, w in S.runs_of(c)]
RUN_IDS = ["%s-%s-h%d%s" % (c["name"], f, h, "" if w is None else "-w%d" % w[0]) for c, f, h, w in RUNS]


def _host(t):
    return t.detach().clone().cpu()


def _make_engine(case, form, heads, window):
    gemm = "f32" if form == "perop_f32" else "x3"
    eng = _engine(S.ITEM_NUM, case["T"], case["H"], case["L"], heads, seed=SEED, gemm=gemm, logits_dtype=case["logits"])
    eng.pack_sessions = form == "packed"
    if window is not None:
        eng.pack_window = window
    sp = case["split"]
    if sp is not None:                                  # a data-parallel shard: train rows and exemplar rows at other global rows
        eng.row0, eng.row0_ex, eng._ex_row0_set = sp["row0"], sp["row0_ex"], True
    assert eng.gemm_x3 == (form != "perop_f32") and eng.seq_fused == (form in ("fused", "packed")) and eng.prune_last
    if form == "perop_x3":
        assert eng.attn_x3 == ((case["H"] // heads) % 2 == 0)
    return eng


def plan_of(A):
    """The device plan of a packed forward's saved activations as numpy arrays (None: not packed)."""
    pk = A.get("pack")
    if pk is None:
        return None
    return {k: pk[k].cpu().numpy() for k in ("hdr", "trows", "ids", "lpos", "gpos", "info", "srow0", "slen")}


def capture_forward(eng, A, form, B, heads, plan):
    """The forward half of a capture: the saved activations A of one forward(save=True) (Engine._act) in the canonical layout of
    oracle/seq_stage_ref.py -> (cap, raw); raw: the tile-ordered (packed) or row-ordered device tensors of the K / V side and of the
    unpruned blocks.  Used by this file's _run and by tests/test_gpu_logits_anchor.py (eval-mode forward)."""
    T, L = eng.T, eng.L
    packed = plan is not None
    tiles = "tiles" if packed else "rows"
    rows = lambda t, lay: S.rows_to_canonical(_host(t), lay, B, T, plan)      # noqa: E731
    cap, raw = {}, {}
    for l in range(L):
        Sd = A[l]
        pruned = Sd["pruned"]
        assert pruned == (l == L - 1)
        ql = "compact" if pruned else tiles
        for k in ("x", "K", "V", "kmask"):
            cap["%s%d" % (k, l)] = rows(Sd[k], tiles)
            raw["%s%d" % (k, l)] = Sd[k]
        for k in ("q_in", "mean1", "std1", "qmask", "Q", "x1", "y", "mean2", "std2", "h1d"):
            cap["%s%d" % (k, l)] = rows(Sd[k], ql)
            if not pruned:
                raw["%s%d" % (k, l)] = Sd[k]
        if pruned:
            play = "last"
        elif packed:
            play = "tiles"
        elif form == "fused" or (form == "perop_x3" and eng.attn_x3):
            play = "kq"
        else:
            play = "qk"
        cap["P%d" % l] = S.p_to_canonical(_host(Sd["P"]), play, B, T, heads, plan)
        if play == "tiles":
            raw["P%d" % l] = Sd["P"]
    cap["x%d" % L] = rows(A["xL"], "compact")
    for k in ("rep", "meanf", "stdf"):
        cap[k] = _host(A[k])
    return cap, raw


def _run(case, form, heads, window, monkeypatch):
    """One loss_and_grad; returns (eng, cfg, prm, cap, plan, raw): the capture in the canonical layout and, for the packed form, the
    device plan and the raw tile-ordered tensors."""
    import ader_amd.engine.backward as BW
    import ader_amd.engine.forward as FW
    batch = S.make_batch(case)
    eng = _make_engine(case, form, heads, window)
    cfg = S.cfg_of(case, batch, heads, SEED, STEP)
    prm = {k: v.float() for k, v in eng.export_params().items()}
    B, T, H, L = cfg["B"], case["T"], case["H"], case["L"]
    packed = form == "packed"
    snaps, launched = [], []
    orig = BW.call
    assert FW.call is orig

    def call(name, *a):
        launched.append(name)
        r = orig(name, *a)
        if name in ("ader_seq_bwd_qkv", "ader_seqp_bwd_qkv"):      # the block-gradient buffers are reused two blocks later
            torch.cuda.synchronize()
            snaps.append({k: _host(eng._ws[k]) for k in ("dx_a", "dx_b", "pdx_a", "pdx_b", "dx_emb") if k in eng._ws})
        return r
    monkeypatch.setattr(BW, "call", call)
    monkeypatch.setattr(FW, "call", call)
    eng.global_step = STEP
    kw = dict(ex_pos=batch["ex_pos"], lambda_=batch["lambda_"]) if batch["ex_pos"] is not None else {}
    eng.loss_and_grad(batch["seq"], batch["pos"], batch["N"], rate=case["rate"], **kw)
    torch.cuda.synchronize()
    eng.check_status()
    monkeypatch.setattr(BW, "call", orig)
    monkeypatch.setattr(FW, "call", orig)
    A, ws = eng._act, eng._ws
    assert (A.get("pack") is not None) == packed
    plan = plan_of(A)
    cap, raw = capture_forward(eng, A, form, B, heads, plan)
    tiles = "tiles" if packed else "rows"
    rows = lambda t, lay: S.rows_to_canonical(_host(t), lay, B, T, plan)      # noqa: E731
    for l in range(L):
        pruned = A[l]["pruned"]
        ql = "compact" if pruned else tiles
        # backward tensors between the chains
        if packed:
            nm = lambda s: "pbw_%s%d%s" % (s, l, "L" if pruned else "")      # noqa: E731
            kv = lambda s: "pbw_%s%d" % (s, l)                                  # noqa: E731
        elif form == "fused":
            nm = kv = lambda s: "bw_%s%d" % (s, l)                              # noqa: E731
        else:
            nm = lambda s: ("bw_dx1" + ("L" if pruned else "")) if s == "dx1" else "bw_%s%d" % (s, l)      # noqa: E731
            kv = lambda s: "bw_%s%d" % (s, l)                                                                  # noqa: E731
        for k in ("dh2", "da", "dx1", "dQ"):
            cap["%s%d" % (k, l)] = rows(ws[nm(k)], ql)
            if not pruned:
                raw["%s%d" % (k, l)] = ws[nm(k)]
        for k in ("dK", "dV"):
            cap["%s%d" % (k, l)] = rows(ws[kv(k)], tiles)
            raw["%s%d" % (k, l)] = ws[kv(k)]
    cap["drep"] = _host(ws["drep"])
    cap["dxo%d" % (L - 1)] = rows(ws["dx_L"], "compact")
    # gradient of block l's input = of block l-1's output: blocks L-1, L-2, .. write the ping-pong buffers b, a, b, ..
    pre = "pdx_" if packed else "dx_"
    for l in range(1, L):
        i = L - 1 - l
        name = pre + ("b" if i % 2 == 0 else "a")
        src = snaps[i][name] if form in ("fused", "packed") else ws[name]
        cap["dxo%d" % (l - 1)] = rows(src, tiles)
        if form in ("fused", "packed"):
            raw["dxo%d" % (l - 1)] = snaps[i][name]
    if form in ("fused", "packed"):
        assert len(snaps) == L
    cap["dxi0"] = rows(eng._last_g, "rows")
    for k in eng.layout:
        cap["g:" + k] = _host(eng.gradient(k))
    return eng, batch, cfg, prm, cap, plan, raw, set(launched)


def expected_launches(case, form, heads):
    """(launchers that must have run, launchers that must not) of a form: the test is about THESE kernels."""
    deep = case["L"] >= 2                        # an unpruned block exists
    if form == "perop_f32":
        must = {"ader_embed_fwd", "ader_ln_fwd", "ader_gemm_rows", "ader_attn_last_fwd", "ader_attn_last_bwd", "ader_mask_dropgrad",
                "ader_ln_bwd", "ader_add_rows", "ader_gemm_atb", "ader_embed_bwd_rows"} | ({"ader_attn_fwd", "ader_attn_bwd"} if deep else set())
        never = {"ader_gemm_x3", "ader_attn_x3_fwd", "ader_attn_x3_bwd", "ader_seq_fwd", "ader_seqp_fwd"}
    elif form == "perop_x3":
        x3 = (case["H"] // heads) % 2 == 0
        core = {"ader_attn_x3_fwd", "ader_attn_x3_bwd"}, {"ader_attn_fwd", "ader_attn_bwd"}
        must = {"ader_embed_fwd", "ader_gemm_x3", "ader_gemm_atb_x3_batch", "ader_attn_last_fwd", "ader_attn_last_bwd", "ader_mask_dropgrad",
                "ader_add_rows", "ader_embed_bwd_rows"} | (core[0 if x3 else 1] if deep else set())
        never = {"ader_gemm_rows", "ader_gemm_atb", "ader_seq_fwd", "ader_seqp_fwd"} | core[1 if x3 else 0]
    elif form == "fused":
        must = {"ader_seq_fwd", "ader_seq_bwd_ffn", "ader_seq_bwd_qkv", "ader_attn_last_bwd", "ader_gemm_atb_x3_batch"} | (
            {"ader_attn_x3_bwd"} if deep else set())
        never = {"ader_seqp_fwd", "ader_embed_fwd", "ader_gemm_x3", "ader_gemm_rows", "ader_attn_bwd"}
    else:
        must = {"ader_seq_pack_plan", "ader_seqp_fwd", "ader_seqp_bwd_ffn", "ader_seqp_bwd_qkv", "ader_attnp_last_bwd",
                "ader_gemm_atb_x3_batch_pk", "ader_pos_grad_packed"} | ({"ader_attnp_bwd"} if deep else set())
        never = {"ader_seq_fwd", "ader_embed_fwd", "ader_gemm_x3", "ader_gemm_rows", "ader_seq_bwd_qkv"}
    if case["logits"] == "x3":                   # the merge launch of the x3 logit forward writes dx of the final LayerNorm
        must, never = must | {"ader_lx3_fwd_img_lnf"}, never | {"ader_ln_bwd"}
    else:
        must, never = must | {"ader_ln_bwd"}, never | {"ader_lx3_fwd_img_lnf"}
    return must, never


def packed_exact_complaints(label, plan, raw, seq, T, window, B, split=None):
    """The exact statements about a packed forward (and whatever backward tensors raw holds): the device plan is numpy_plan of
    seq [B, T]; no tile row at or beyond its tile's row count and no saved probability outside its session's causal block was written.
    raw is consumed.  -> complaints."""
    complaints = []
    sp = split
    ref_plan = numpy_plan(seq, T, window, sp["row0"] if sp else 0, sp["n_train"] if sp else -1, sp["row0_ex"] if sp else 0)
    nt = int(ref_plan["hdr"][0])
    ok = np.array_equal(plan["hdr"][:4], ref_plan["hdr"]) and np.array_equal(plan["trows"][:nt], ref_plan["tile_rows"])
    ok = ok and np.array_equal(plan["srow0"], ref_plan["srow0"]) and np.array_equal(plan["slen"], ref_plan["slen"])
    used = ref_plan["ids"] >= 0
    for k in ("ids", "lpos", "gpos", "info"):
        ok = ok and np.array_equal(plan[k][:nt * 64][used].astype(np.int64), ref_plan[k][used])
    if not ok:
        complaints.append("%s device plan differs from numpy_plan" % label)
    # rows at or beyond a tile's row count: allocated zeroed, never written
    tr = np.zeros(B, dtype=np.int64)
    tr[:nt] = ref_plan["tile_rows"]
    beyond = torch.from_numpy((np.arange(64)[None, :] >= tr[:, None]).reshape(-1))
    dirty = []
    # ... and of the saved probabilities [tile][key][query] everything but a session's own causal block
    own = torch.zeros(B, 64, 64, dtype=torch.bool)
    for b in range(B):
        u, r0 = divmod(int(ref_plan["srow0"][b]), 64)
        n = int(ref_plan["slen"][b])
        own[u, r0:r0 + n, r0:r0 + n] = torch.triu(torch.ones(n, n, dtype=torch.bool))       # key <= query
    for k in [k for k in raw if k.startswith("P")]:
        Pt = _host(raw.pop(k)).reshape(B, 64, 64).view(torch.int32)
        if bool((Pt[~own] != 0).any()):
            complaints.append("%s %s: a probability outside its session's causal block was written" % (label, k))
    for k, t in raw.items():
        t = _host(t) if t.is_cuda else t
        t2 = t.reshape(B * 64, -1).contiguous().view(torch.int32)
        if bool((t2[beyond] != 0).any()):
            dirty.append(k)
    if dirty:
        complaints.append("%s tile rows beyond the tile's row count were written: %s" % (label, ", ".join(sorted(dirty))))
    return complaints


@pytest.mark.parametrize("case,form,heads,window", RUNS, ids=RUN_IDS)
def test_every_stage_matches_its_float64_restatement(case, form, heads, window, monkeypatch):
    eng, batch, cfg, prm, cap, plan, raw, launched = _run(case, form, heads, window, monkeypatch)
    must, never = expected_launches(case, form, heads)
    assert must <= launched and not (never & launched), (sorted(must - launched), sorted(never & launched))
    assert eng.lx3 == (case["logits"] == "x3")
    B, T, H, L, N = cfg["B"], case["T"], case["H"], case["L"], batch["N"]
    real = cfg["real"]
    label = "%s %s h%d%s" % (case["name"], form, heads, "" if window is None else " w%d" % window[0])
    rows, bad, ref = S.check_capture(cap, cfg, prm, form, raise_=False)
    for line in S.format_rows(rows, label):
        print(line)
    complaints = list(bad)
    # every output of every stage was judged (the masks are judged exactly, below)
    judged = {(st, l, nm) for st, l, nm, *_ in rows}
    wanted = {(st, l, nm) for (st, l), (out, _) in ref.items() for nm in out if nm not in ("kmask", "qmask")}
    assert judged == wanted, sorted(wanted ^ judged)
    # ---- exact checks
    for l in range(L):
        qp = S.qpos_of(cfg, l)
        if not bool((cap["kmask%d" % l][real] == 1.0).all()):
            complaints.append("%s kmask block %d is not 1.0 at every real row" % (label, l))
        if not bool((cap["qmask%d" % l][real[:, qp]] == 1.0).all()):
            complaints.append("%s qmask block %d is not 1.0 at every real row" % (label, l))
        keep1 = S.keep_mask(cfg, S.R.site_ffn1(l), (T, H))[:, qp]
        dropped = (~keep1) & real[:, qp].unsqueeze(-1)
        if not bool((cap["h1d%d" % l][dropped] == 0).all()):
            complaints.append("%s h1d block %d: a dropped element is not zero" % (label, l))
    x0_ref = ref[("embed", 0)][0]["x0"]
    m = real.unsqueeze(-1).expand_as(x0_ref)
    if not torch.equal(cap["x0"][m] == 0, x0_ref[m] == 0):
        complaints.append("%s x0: zero pattern differs from the dropout decisions" % label)
    if not bool((cap["x0"][~real] == 0).all()):
        complaints.append("%s x0: a padding position is not zero" % label)
    lnf_b = prm["lnf_b"]
    for b in torch.nonzero(~real.any(1)).reshape(-1).tolist():
        if not torch.equal(cap["rep"][b], lnf_b):
            complaints.append("%s rep of the all-padding session %d is not the final LayerNorm's beta" % (label, b))
    demb = cap["g:emb"]
    if not (bool((demb[0] == 0).all()) and bool((demb[N + 1:] == 0).all())):
        complaints.append("%s table gradient: row 0 or a row beyond max_item is not zero" % label)
    if plan is not None:
        complaints += packed_exact_complaints(label, plan, raw, batch["seq"], T, window, B, case["split"])
    assert not complaints, "\n".join(complaints)
