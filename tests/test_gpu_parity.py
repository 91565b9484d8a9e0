"""GPU parity tests: the HIP path (through the C ABI, libader_hip.so) against the CPU oracle on the same seeded
inputs.  Floating point: tolerance stated per test (float32 kernels vs float32/float64 oracle; differences are
summation order and exp/log ulps only).  Index work (ranks from identical logits, herding) is bit-exact."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))

from oracle import ader_ref_cpu as R  # noqa: E402
from oracle import herding_ref  # noqa: E402


def _engine(item_num, T, H, L, heads, seed=0, **kw):
    from ader_amd.engine import Engine
    kw.setdefault("logits_dtype", "f32")      # the exact-f32 kernels unless a test names another arithmetic (Engine's default is "x3")
    eng = Engine(item_num, maxlen=T, hidden_units=H, num_blocks=L, num_heads=heads, seed=seed, **kw)
    # non-trivial LN parameters / biases so masks and residual paths are exercised away from the init symmetry
    g = torch.Generator().manual_seed(seed + 11)
    for k in eng.layout:
        base = k.split(".")[-1]
        shp = eng.layout[k][1]
        if base.endswith("_b") or base in ("bq", "bk", "bv", "b1", "b2"):
            eng.param(k).copy_(torch.randn(shp, generator=g) * 0.1)
        elif base.endswith("_g"):
            eng.param(k).copy_(1 + torch.randn(shp, generator=g) * 0.1)
        elif base in ("wq", "wk", "wv", "w1", "w2"):
            eng.param(k).copy_(torch.randn(shp, generator=g) * (1.0 / np.sqrt(shp[0])))
        elif base == "emb":
            eng.param(k).copy_(torch.randn(shp, generator=g) * 0.05)
    eng.refresh_shadow()
    return eng


def _params(eng, dtype):
    return {k: v.to(dtype) for k, v in eng.export_params().items()}


def _seqs(rs, B, T, n_items, full=False):
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = T if full else int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


def relu_masks_of(eng):
    """The ReLU/dropout branch decisions the device took in the last training forward (see oracle forward_rep)."""
    out = {}
    for l in range(eng.L):
        S = eng._act[l]
        out[l] = ("last" if S["pruned"] else "all", (S["h1d"] != 0).cpu())
    return out


def assert_shadow_is_bf16_of_theta(eng):
    """The bf16 shadow of the table behind whatever kernel wrote it last: shadow[:, :H] == bf16(theta) BITWISE, padding columns zero."""
    sh = eng.shadow.view(-1, 168)[:eng.V].cpu()
    emb = eng.param("emb").cpu()
    assert torch.equal(sh[:, :eng.H].contiguous().view(torch.int16), emb.bfloat16().view(torch.int16))
    assert not bool((sh[:, eng.H:].contiguous().view(torch.int16) != 0).any())


def nerr(a, b, floor=0.0):
    """max |a-b| normalised by max(|b|max, floor).  `floor` guards tensors whose true value is ~0 (e.g. the key bias
    gradient: softmax is shift-invariant, so d/d(bk) is exactly zero up to float32 noise)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor, 1e-30))


CFGS = [  # item_num, T, H, L, heads, B, N
    (700, 50, 150, 2, 1, 70, 650),
    (300, 20, 64, 1, 2, 9, 300),
    (1000, 50, 150, 2, 3, 130, 777),
]


def test_library_loads_and_runs():
    from ader_amd import _lib
    _lib.load()
    t = torch.zeros(1000, device="cuda")
    _lib.call("ader_fill", t.data_ptr(), 1000, 3.5, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.all(t == 3.5)


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("rate", [0.0, 0.3])
def test_forward_matches_oracle(cfg, rate):
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(1)
    seq = _seqs(rs, B, T, N)
    rep = eng.forward(eng._dev_i32(seq), training=rate > 0, rate=rate, step=5, save=True)
    torch.cuda.synchronize()
    ref, inter = R.forward_rep(_params(eng, torch.float64), seq, L, heads, training=rate > 0, rate=rate, seed=0, step=5,
                               return_intermediates=True)
    A = eng._act
    real = torch.from_numpy(seq != 0)
    # tolerance: float32 kernels vs float64 oracle, normalised max error
    assert nerr(A[0]["x"].cpu().view(B, T, H), inter["x0"]) < 1e-5
    if A[0]["pruned"]:                                             # single-block model: only row T-1 is computed
        assert nerr(A[0]["x1"].cpu(), inter["attn0"][:, -1]) < 5e-5
    else:
        x1 = A[0]["x1"].cpu().view(B, T, H)
        assert nerr(x1[real], inter["attn0"][real]) < 5e-5        # pad rows are re-zeroed by the mask (ADER.py:80)
    assert nerr(rep.cpu(), ref) < 1e-4
    eng.check_status()


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("mode", ["vanilla", "kd", "onehot_ex"])
@pytest.mark.parametrize("gemm", ["x3", "f32"])
def test_loss_and_gradients_match_oracle(cfg, mode, gemm):
    """gemm="f32": exact f32 MFMA kernels; gemm="x3": bf16 hi/lo split (3 bf16 MFMAs per product, fp32 accumulate),
    GEMMs and attention core.  Float32-level tolerances against the float64 oracle (3e-4 / 6e-4 normalised)."""
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads, seed=3, gemm=gemm)
    rs = np.random.RandomState(2)
    seq = _seqs(rs, B, T, N)
    n_ex = 0 if mode == "vanilla" else max(1, B // 4)
    n_train = B - n_ex
    pos = rs.randint(1, N + 1, size=n_train).astype(np.int32)
    kw, okw = {}, {}
    lam = 0.45
    if mode == "kd":
        Np = N - 37
        store = torch.from_numpy(rs.standard_normal((n_ex + 5, Np)).astype(np.float32) * 2).cuda()
        trow = rs.permutation(n_ex + 5)[:n_ex].astype(np.int32)
        kw = dict(teacher=store, ex_trow=trow, lambda_=lam)
        okw = dict(ex_logits=store.cpu()[trow.astype(np.int64)].double(), lambda_=lam)
    elif mode == "onehot_ex":
        ex_pos = rs.randint(1, N + 1, size=n_ex).astype(np.int32)
        kw = dict(ex_pos=ex_pos, lambda_=lam)
        okw = dict(ex_pos=ex_pos, lambda_=lam)
    eng.global_step = 4
    loss = eng.loss_and_grad(seq, pos, N, rate=0.3, **kw)
    torch.cuda.synchronize()
    eng.check_status()
    # x3: compare on the device's own ReLU branch decisions (pre-activations within 2^-16 of zero may take the other
    # branch than the float64 oracle; see oracle.forward_rep).  f32: the plain oracle.
    masks = relu_masks_of(eng) if gemm == "x3" else None
    oloss, og = R.loss_and_grads(_params(eng, torch.float64), seq, pos, N, L, heads, training=True, rate=0.3, seed=3, step=4,
                                 relu_masks=masks, **okw)
    assert abs(float(loss.item()) - float(oloss)) < 2e-5 * max(1.0, abs(float(oloss)))
    worst = {}
    for k in eng.layout:
        g = eng.gradient(k).cpu().numpy()
        e = nerr(g, og[k].numpy(), floor=1e-4)
        worst[k] = e
        # float64 oracle vs: exact f32 MFMA kernels (measured ~1e-6) -> 3e-4; bf16x3 kernels (2^-16 per product through
        # two blocks of GEMMs + attention) -> 6e-4
        assert e < (6e-4 if gemm == "x3" else 3e-4), (k, e)
    assert np.all(eng.gradient("emb")[0].cpu().numpy() == 0)        # row 0 never receives gradient (modules.py:124-126)
    assert np.all(eng.gradient("emb")[N + 1:].cpu().numpy() == 0)   # items beyond max_item are outside the softmax
    if gemm == "x3":
        _check_against_plain_oracle(eng, masks, seq, pos, N, L, heads, okw, float(loss.item()))


def flipped_relu_fraction(dev_masks, inter, seq):
    """Fraction of ReLU/dropout branch decisions (real positions only; row T-1 for a pruned block) on which the device and
    the float64 oracle disagree."""
    real = torch.from_numpy(np.asarray(seq) != 0)
    bad = tot = 0
    for l, (kind, mk) in dev_masks.items():
        o = inter["h1d%d" % l] != 0
        if kind == "all":
            d = mk.view(o.shape)
            sel = real
        else:
            o, d = o[:, -1], mk.view(o.shape[0], o.shape[2])
            sel = real[:, -1]
        bad += int((o[sel] != d[sel]).sum())
        tot += int(o[sel].numel())
    return bad / max(tot, 1)


def _check_against_plain_oracle(eng, masks, seq, pos, N, L, heads, okw, got_loss, step=4, seed=3):
    """The default (bf16x3) path against the PLAIN float64 oracle -- no branch decisions handed over.  Stated, looser
    bounds: the device may take the other ReLU branch only where the pre-activation is within its ~2^-16 rounding of zero
    (fraction of disagreeing decisions < 1e-3), and each such flip moves individual gradient entries by O(1e-3)
    (every gradient tensor within 1e-2 normalised -- measured up to 5.7e-3 -- and the loss within 2e-5).  A wrong mask (a real bug) violates the first bound
    by orders of magnitude: tests/test_gpu_parity.py::test_plain_oracle_check_catches_a_wrong_mask."""
    p64 = _params(eng, torch.float64)
    _, inter = R.forward_rep(p64, seq, L, heads, training=True, rate=0.3, seed=seed, step=step, return_intermediates=True)
    frac = flipped_relu_fraction(masks, inter, seq)
    assert frac < 1e-3, ("ReLU/dropout decisions differ from the plain oracle", frac)
    oloss, og = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=seed, step=step, **okw)
    assert abs(got_loss - float(oloss)) < 2e-5 * max(1.0, abs(float(oloss)))
    for k in eng.layout:
        e = nerr(eng.gradient(k).cpu().numpy(), og[k].numpy(), floor=1e-4)
        assert e < 1e-2, (k, "vs plain oracle", e)


def test_plain_oracle_check_catches_a_wrong_mask():
    """The plain-oracle assertion must fail when the device's branch decisions are wrong: invert one session's decisions."""
    item_num, T, H, L, heads, B, N = CFGS[0]
    eng = _engine(item_num, T, H, L, heads, seed=3, gemm="x3")
    rs = np.random.RandomState(2)
    seq = _seqs(rs, B, T, N, full=True)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    eng.global_step = 4
    loss = eng.loss_and_grad(seq, pos, N, rate=0.3)
    torch.cuda.synchronize()
    masks = relu_masks_of(eng)
    _check_against_plain_oracle(eng, masks, seq, pos, N, L, heads, {}, float(loss.item()))     # the real masks pass
    kind, mk = masks[0]
    bad = mk.clone().view(B, -1)
    bad[0] = ~bad[0]
    with pytest.raises(AssertionError):
        _check_against_plain_oracle(eng, {**masks, 0: (kind, bad.view(mk.shape))}, seq, pos, N, L, heads, {}, float(loss.item()))


BF16_CFGS = [  # item_num, T, H, L, heads, B, N  (tail tiles, several ranges, B not a multiple of 128, empty ranges)
    (700, 50, 150, 2, 1, 70, 650),
    (5000, 50, 150, 1, 1, 300, 4321),
    (300, 20, 64, 1, 2, 9, 300),
]


@pytest.mark.parametrize("cfg", BF16_CFGS)
@pytest.mark.parametrize("mode", ["vanilla", "onehot_ex"])
def test_bf16_logits_path_matches_bf16_aware_oracle(cfg, mode):
    """bf16-MFMA logits mode.  Checked (a) tightly against the oracle evaluated with the same operand rounding
    (rep and table rounded to bf16 inside the logits product, straight-through gradient): remaining differences are the
    bf16 rounding of the probabilities fed to the second MFMA (relative 2^-9 = 2e-3 per element) and summation
    order -> 6e-3 normalised; and
    (b) loosely against the exact float64 oracle: 3e-2 normalised, loss within 5e-3 relative (bf16 operand rounding)."""
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads, seed=3, logits_dtype="bf16")
    rs = np.random.RandomState(12)
    seq = _seqs(rs, B, T, N)
    n_ex = 0 if mode == "vanilla" else max(1, B // 4)
    n_train = B - n_ex
    pos = rs.randint(1, N + 1, size=n_train).astype(np.int32)
    pos[0] = N                                    # a label in the tail tile
    kw, okw = {}, {}
    if mode == "onehot_ex":
        ex_pos = rs.randint(1, N + 1, size=n_ex).astype(np.int32)
        kw = dict(ex_pos=ex_pos, lambda_=0.6)
        okw = dict(ex_pos=ex_pos, lambda_=0.6)
    eng.global_step = 2
    loss = eng.loss_and_grad(seq, pos, N, rate=0.3, **kw)
    torch.cuda.synchronize()
    eng.check_status()
    p64 = _params(eng, torch.float64)
    mk = relu_masks_of(eng)
    l_q, g_q = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=3, step=2, logits_bf16=True,
                                relu_masks=mk, **okw)
    l_x, g_x = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=3, step=2, relu_masks=mk, **okw)
    got = float(loss.item())
    assert abs(got - float(l_q)) < 3e-4 * max(1.0, abs(float(l_q)))
    assert abs(got - float(l_x)) < 5e-3 * max(1.0, abs(float(l_x)))
    for k in eng.layout:
        g = eng.gradient(k).cpu().numpy()
        eq = nerr(g, g_q[k].numpy(), floor=1e-4)
        ex = nerr(g, g_x[k].numpy(), floor=1e-4)
        assert eq < 6e-3, (k, "vs bf16-aware oracle", eq)
        assert ex < 3e-2, (k, "vs exact oracle", ex)
    assert np.all(eng.gradient("emb")[0].cpu().numpy() == 0)
    assert np.all(eng.gradient("emb")[N + 1:].cpu().numpy() == 0)


@pytest.mark.parametrize("cfg", BF16_CFGS)
@pytest.mark.parametrize("mode", ["vanilla", "onehot_ex"])
@pytest.mark.parametrize("gemm", ["f32", "x3"])
def test_x3_logits_path_matches_exact_oracle(cfg, mode, gemm):
    """logits_dtype="x3": the flash logit kernels with every product as three bf16 MFMAs on hi/lo operand splits (fp32
    accumulate): float32-grade, so it is held to the SAME bounds as the exact-f32 kernels against the plain float64 oracle
    (no bf16-aware oracle): loss 2e-6, every gradient 5e-5 normalised with exact-f32 block GEMMs (6e-4 with the bf16x3 block
    GEMMs, which are handed their own ReLU decisions as in test_loss_and_gradients_match_oracle).  Reference arithmetic:
    ADER.py:91-93 (fp32)."""
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads, seed=3, logits_dtype="x3", gemm=gemm)
    assert eng.shadow is None and eng.lx3
    rs = np.random.RandomState(12)
    seq = _seqs(rs, B, T, N)
    n_ex = 0 if mode == "vanilla" else max(1, B // 4)
    n_train = B - n_ex
    pos = rs.randint(1, N + 1, size=n_train).astype(np.int32)
    pos[0] = N                                    # a label in the tail tile
    kw, okw = {}, {}
    if mode == "onehot_ex":
        ex_pos = rs.randint(1, N + 1, size=n_ex).astype(np.int32)
        kw = dict(ex_pos=ex_pos, lambda_=0.6)
        okw = dict(ex_pos=ex_pos, lambda_=0.6)
    eng.global_step = 2
    loss = eng.loss_and_grad(seq, pos, N, rate=0.3, **kw)
    torch.cuda.synchronize()
    eng.check_status()
    masks = relu_masks_of(eng) if gemm == "x3" else None
    ol, og = R.loss_and_grads(_params(eng, torch.float64), seq, pos, N, L, heads, training=True, rate=0.3, seed=3, step=2,
                              relu_masks=masks, **okw)
    # (round 6: bounds from what is measured -- loss 1.5e-7; gradients 1.2e-5 with exact-f32 block GEMMs, worst on the key bias, whose
    #  true gradient is zero and which is normalised by the 1e-4 floor; up to 4.1e-4 on that same tensor with the bf16x3 block GEMMs)
    assert abs(float(loss.item()) - float(ol)) < 2e-6 * max(1.0, abs(float(ol)))
    worst = ("", 0.0)
    for k in eng.layout:
        e = nerr(eng.gradient(k).cpu().numpy(), og[k].numpy(), floor=1e-4)
        worst = max(worst, (k, e), key=lambda t: t[1])
        assert e < (6e-4 if gemm == "x3" else 5e-5), (k, e)
    print("x3 logits path, %s / %s block GEMMs: loss err %.2e, worst gradient %s %.2e" % (
        mode, gemm, abs(float(loss.item()) - float(ol)) / max(1.0, abs(float(ol))), worst[0], worst[1]))
    assert np.all(eng.gradient("emb")[0].cpu().numpy() == 0)
    assert np.all(eng.gradient("emb")[N + 1:].cpu().numpy() == 0)


def test_x3_train_steps_track_the_oracle():
    """Three fused train steps (x3 flash forward, x3 table-gradient GEMM + sparse terms + Adam in one kernel) against the
    float32 oracle with TF-Adam: same bounds as the exact-f32 path (test_three_train_steps_track_the_oracle)."""
    item_num, T, H, L, heads, B, N = CFGS[0]
    eng = _engine(item_num, T, H, L, heads, seed=7, logits_dtype="x3")
    params = _params(eng, torch.float32)
    opt = R.TFAdam(params)
    rs = np.random.RandomState(4)
    for it in range(3):
        seq = _seqs(rs, B, T, N)
        pos = rs.randint(1, N + 1, size=B).astype(np.int32)
        loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3)
        ol = R.train_step(params, opt, seq, pos, N, L, heads, 5e-4, training=True, rate=0.3, seed=7, step=it)
        assert abs(float(loss.item()) - ol) < 1e-4 * max(1.0, abs(ol))
    for k in eng.layout:
        d = np.abs(eng.param(k).cpu().numpy() - params[k].numpy()).max()
        assert d < 3e-4, (k, d)


def test_full_last_block_equals_pruned_last_block():
    """Engine.prune_last computes only position T-1 of the final block; the unpruned path (all T rows, as the reference
    graph does) must give the same loss and gradients."""
    item_num, T, H, L, heads, B, N = CFGS[2]
    rs = np.random.RandomState(21)
    seq = _seqs(rs, B, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    out = []
    for prune in (True, False):
        eng = _engine(item_num, T, H, L, heads, seed=5)
        eng.prune_last = prune
        eng.global_step = 1
        loss = eng.loss_and_grad(seq, pos, N, rate=0.3)
        torch.cuda.synchronize()
        out.append((float(loss.item()), {k: eng.gradient(k).cpu().numpy().copy() for k in eng.layout}))
    assert abs(out[0][0] - out[1][0]) < 1e-6
    for k in out[0][1]:
        # same arithmetic per row either way; differences are summation order of the row reductions (floor 1e-4
        # covers the key-bias gradient, which is zero up to rounding noise)
        assert nerr(out[0][1][k], out[1][1][k], floor=1e-4) < 5e-4, k


@pytest.mark.parametrize("shape", [(700, 50, 150, 2, 70, 650), (400, 64, 150, 1, 5, 400), (300, 7, 64, 3, 33, 250)])
@pytest.mark.parametrize("prune", [True, False])
def test_one_launch_forward_equals_per_op_forward(shape, prune):
    """ader_seq_fwd (whole stack per session in one workgroup) writes the same representation and the same saved
    activations as the chain of per-op kernels it replaces: identical arithmetic per element (bf16x3 products, fp32
    LayerNorm / softmax), identical dropout masks; differences are fp32 rounding of differently ordered MFMA k-steps."""
    item_num, T, H, L, B, N = shape
    rs = np.random.RandomState(3)
    seq = _seqs(rs, B, T, N)
    seq[0, :] = 0                                 # an all-padding session
    seq[1, :-1] = 0                               # a single-item session
    acts = []
    for fused in (True, False):
        eng = _engine(item_num, T, H, L, 1, seed=9)
        assert eng.seq_fused
        eng.seq_fused = fused
        eng.prune_last = prune
        rep = eng.forward(eng._dev_i32(seq), training=True, rate=0.3, step=2, save=True)
        torch.cuda.synchronize()
        A = eng._act
        d = {"rep": rep.cpu().numpy().copy(), "meanf": A["meanf"].cpu().numpy().copy(), "stdf": A["stdf"].cpu().numpy().copy(),
             "xL": A["xL"].cpu().numpy().copy()}
        for l in range(L):
            for k2, v in A[l].items():
                if isinstance(v, torch.Tensor):
                    d["%d.%s" % (l, k2)] = v.cpu().numpy().copy()
        acts.append(d)
    assert acts[0].keys() == acts[1].keys()
    # Leading padding rows: the one-launch kernel skips them (their keys are masked, their outputs re-zeroed, their gradient is
    # exactly zero: nothing consumes what the per-op chain computes there), so their saved rows are unspecified -- compared from the
    # first real position on.  Compact tensors of a pruned block hold row T-1 (padding only in the all-padding session).
    tv0 = np.array([int(np.argmax(r != 0)) if (r != 0).any() else T for r in seq])
    padrow = (np.arange(T)[None, :] < tv0[:, None])                      # [B, T]

    def drop_pad(x, k2):
        x = x.copy()
        if k2.endswith(".P") and x.size == B * T * T:                   # P^T [b][key][query]: padding QUERIES
            x.reshape(B, T, T)[np.broadcast_to(padrow[:, None, :], (B, T, T))] = 0
        elif x.shape[0] == B * T:
            x.reshape(B, T, -1)[padrow] = 0
        elif x.shape[0] == B and k2 not in ("rep", "meanf", "stdf"):
            x.reshape(B, -1)[tv0 == T] = 0
        elif k2.endswith(".P") and x.size == B * T:                     # pruned: the row of query T-1
            x.reshape(B, T)[tv0 == T] = 0
        return x

    for k2 in acts[0]:
        a, b = drop_pad(acts[0][k2], k2), drop_pad(acts[1][k2], k2)
        assert a.shape == b.shape, k2
        if k2.endswith("mask"):
            assert np.array_equal(a, b), k2
        elif k2.endswith(".h1d"):
            # a pre-activation within rounding of zero may take the other ReLU branch
            same = (a != 0) == (b != 0)
            assert np.mean(~same) < 1e-3, k2
            assert nerr(np.where(same, a, 0), np.where(same, b, 0), floor=1e-3) < 1e-4, k2
        else:
            # 1e-4: the per-op path evaluates the pruned block's single-query attention with exact f32 FMAs, the fused kernel
            # with bf16x3 products (2^-16 relative each); everything else agrees to ~1e-6
            assert nerr(a, b, floor=1e-3) < 1e-4, (k2, nerr(a, b, floor=1e-3))


@pytest.mark.parametrize("shape", [(700, 50, 150, 2, 70, 650), (400, 64, 150, 1, 5, 400), (300, 7, 64, 3, 33, 250)])
@pytest.mark.parametrize("prune", [True, False])
def test_session_tiled_step_equals_per_op_step(shape, prune):
    """Loss and every gradient from the session-tiled kernels (ader_seq_fwd, ader_seq_bwd_ffn, ader_seq_bwd_qkv) against the
    per-op kernel chain they replace, same parameters, inputs and dropout masks."""
    item_num, T, H, L, B, N = shape
    rs = np.random.RandomState(4)
    seq = _seqs(rs, B, T, N)
    seq[0, :] = 0
    seq[1, :-1] = 0
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    out = []
    for fused in (True, False):
        eng = _engine(item_num, T, H, L, 1, seed=9)
        eng.seq_fused = fused
        eng.prune_last = prune
        eng.global_step = 3
        loss = eng.loss_and_grad(seq, pos, N, rate=0.3)
        torch.cuda.synchronize()
        out.append((float(loss.item()), {k: eng.gradient(k).cpu().numpy().copy() for k in eng.layout},
                    eng._last_g.cpu().numpy().copy()))
    assert abs(out[0][0] - out[1][0]) < 2e-5 * max(1.0, abs(out[1][0]))
    assert nerr(out[0][2], out[1][2], floor=1e-6) < 2e-3        # per-position input-gradient rows
    for k in out[0][1]:
        # differences: fp32 summation order, ReLU branch flips of ~zero pre-activations (cf. the x3 oracle test: 6e-4).
        # The key bias has an exactly-zero true gradient (softmax is shift invariant): both paths hold ~1e-8 rounding noise
        fl = 1e-3 if k.endswith(".bk") else 1e-4
        assert nerr(out[0][1][k], out[1][1][k], floor=fl) < 6e-4, (k, nerr(out[0][1][k], out[1][1][k], floor=fl))


def test_stale_rows_of_skipped_padding_are_harmless():
    """The session-tiled kernels skip a session's leading padding rows (forward: nothing stored; backward: zero gradient rows written).
    What the activation buffers hold there is stale -- here: the rows of a previous step whose sessions were LONGER, scaled up to
    1e3 to make any leak visible.  Loss and every gradient of the second step must equal the per-op chain's, which computes every
    row."""
    item_num, T, H, L, B, N = 700, 50, 150, 2, 70, 650
    rs = np.random.RandomState(12)
    long_seq = _seqs(rs, B, T, N, full=True)
    short_seq = np.zeros_like(long_seq)
    for b in range(B):
        ln = 1 + b % 19                               # 1 .. 19 items: some sessions reach into rows < 32, most do not
        short_seq[b, T - ln:] = rs.randint(1, N + 1, size=ln)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    out = []
    for fused in (True, False):
        eng = _engine(item_num, T, H, L, 1, seed=9)
        eng.seq_fused = fused
        eng.global_step = 3
        eng.loss_and_grad(long_seq, pos, N, rate=0.3)
        torch.cuda.synchronize()
        if fused:                                     # blow up what step 1 left in the saved-activation buffers
            for name, t in eng._ws.items():
                if t.dtype == torch.float32 and name[:1] == "t" and t.dim() == 2:
                    t.mul_(1e3)
        eng.global_step = 4
        loss = eng.loss_and_grad(short_seq, pos, N, rate=0.3)
        torch.cuda.synchronize()
        out.append((float(loss.item()), {k: eng.gradient(k).cpu().numpy().copy() for k in eng.layout},
                    eng._last_g.cpu().numpy().copy()))
    assert np.isfinite(out[0][0]) and abs(out[0][0] - out[1][0]) < 2e-5 * max(1.0, abs(out[1][0]))
    assert nerr(out[0][2], out[1][2], floor=1e-6) < 2e-3
    for k in out[0][1]:
        fl = 1e-3 if k.endswith(".bk") else 1e-4
        assert np.isfinite(out[0][1][k]).all(), k
        assert nerr(out[0][1][k], out[1][1][k], floor=fl) < 6e-4, (k, nerr(out[0][1][k], out[1][1][k], floor=fl))


@pytest.mark.parametrize("N,shards", [(4321, 2), (4321, 3), (650, 8)])
def test_sharded_logits_forward_equals_unsharded(N, shards):
    """Catalog-sharded softmax (ader_lbf_fwd_shard per item shard + ader_lbf_merge_parts) against ader_lbf_fwd over the whole
    catalog on the same bf16 operands: lse, backward offsets, loss rows and dRep.  Shards beyond N are empty partials."""
    from ader_amd._lib import call, ptr
    item_num, H, B = 5000, 150, 200
    Bp = 256
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(N)
    emb = (torch.randn(item_num + 1, H, generator=g) * 0.05).to(dev)
    rep = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    lab = torch.zeros(Bp, dtype=torch.int32, device=dev)
    lab[:B] = torch.randint(1, N + 1, (B,), generator=g).to(dev)
    wrow = torch.zeros(Bp, device=dev)
    wrow[:B] = 1.0 / B
    shadow = torch.zeros((item_num + 1) * 168, dtype=torch.bfloat16, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    call("ader_lbf_shadow_refresh", ptr(emb), ptr(shadow), item_num + 1, H, st)
    rep_bf = torch.zeros(Bp * 168, dtype=torch.bfloat16, device=dev)
    R = call("ader_lbf_ranges", N, Bp)
    pm, pl, pO = torch.empty(R * Bp, device=dev), torch.empty(R * Bp, device=dev), torch.empty(R * Bp * 160, device=dev)
    ref = {k: torch.zeros(Bp, device=dev) for k in ("lse", "off", "rowloss")}
    loss, drep = torch.zeros(1, device=dev), torch.zeros(B, H, device=dev)
    call("ader_lbf_fwd", ptr(rep), ptr(shadow), item_num, B, Bp, H, N, ptr(lab), ptr(wrow), ptr(rep_bf), ptr(pm), ptr(pl), ptr(pO),
         ptr(ref["lse"]), ptr(ref["off"]), ptr(ref["rowloss"]), ptr(loss), ptr(drep), st)
    S = -(-item_num // (128 * shards)) * 128
    parts = torch.empty(shards, Bp, 152, device=dev)
    call("ader_lbf_prep", ptr(rep), ptr(rep_bf), B, Bp, H, st)
    Rs = call("ader_lbf_ranges", S, Bp)
    pm2, pl2, pO2 = torch.empty(Rs * Bp, device=dev), torch.empty(Rs * Bp, device=dev), torch.empty(Rs * Bp * 160, device=dev)
    for r in range(shards):
        call("ader_lbf_fwd_shard", ptr(rep_bf), ptr(shadow), item_num, Bp, H, N, r * S, S, ptr(pm2), ptr(pl2), ptr(pO2),
             ptr(parts[r]), st)
    e_lab = emb[lab[:B].long()].contiguous()
    got = {k: torch.zeros(Bp, device=dev) for k in ("lse", "off", "rowloss")}
    loss2, drep2 = torch.zeros(1, device=dev), torch.zeros(B, H, device=dev)
    call("ader_lbf_merge_parts", ptr(parts), shards, Bp, B, H, ptr(e_lab), ptr(rep_bf), ptr(wrow), ptr(got["lse"]), ptr(got["off"]),
         ptr(got["rowloss"]), ptr(loss2), ptr(drep2), st)
    torch.cuda.synchronize()
    for k in ref:      # same bf16 products, fp32 sums in a different grouping
        a, b = got[k][:B].cpu().numpy(), ref[k][:B].cpu().numpy()
        assert nerr(a, b) < 2e-6, (k, nerr(a, b))
    assert np.all(np.isneginf(got["off"][B:].cpu().numpy()))
    assert abs(float(loss2) - float(loss)) < 2e-6 * abs(float(loss))
    assert nerr(drep2.cpu().numpy(), drep.cpu().numpy()) < 2e-5


def test_owned_rows_travel_between_shards():
    """ader_gather_owned / ader_scatter_owned: every input position's table row is produced by exactly one shard and lands in
    the receiver's table (labels in the side buffer); padding ids are skipped.  Index work: exact."""
    from ader_amd._lib import call, ptr
    V, H, W, S, n_tab, n_lab = 1025, 6, 4, 256, 300, 20
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    table = torch.randn(V, H, generator=g).to(dev)
    ids = torch.randint(0, V, (n_tab + n_lab,), generator=g, dtype=torch.int32)
    ids[:7] = 0
    ids = ids.to(dev)
    n = n_tab + n_lab
    st = torch.cuda.current_stream().cuda_stream
    recv = torch.empty(W, n, H, device=dev)
    for r in range(W):                       # what rank r would send for these positions
        call("ader_gather_owned", ptr(table), ptr(ids), n, H, r * S, (r + 1) * S, ptr(recv[r]), st)
    assert torch.equal(recv.sum(0), table[ids.long()] * (ids > 0).unsqueeze(-1))
    dst = torch.full((V, H), -1.0, device=dev)
    extra = torch.full((n_lab, H), -1.0, device=dev)
    call("ader_scatter_owned", ptr(recv), ptr(ids), n, n_tab, H, S, W, ptr(dst), ptr(extra), st)
    torch.cuda.synchronize()
    t_ids = ids[:n_tab].long()
    live = t_ids[t_ids > 0]
    assert torch.equal(dst[live], table[live])
    untouched = torch.ones(V, dtype=torch.bool, device=dev)
    untouched[live] = False
    assert torch.all(dst[untouched] == -1.0)
    assert torch.equal(extra, table[ids[n_tab:].long()] * (ids[n_tab:] > 0).unsqueeze(-1))


@pytest.mark.parametrize("cfg", [BF16_CFGS[0], BF16_CFGS[1]])
@pytest.mark.parametrize("ld", ["bf16", "x3"])
def test_fused_table_adam_equals_unfused_step(cfg, ld):
    """Engine.fuse_adam applies Adam to the item table inside the table-gradient kernel (dE never written to memory,
    sparse terms added from id-sorted lists).  Two steps must leave the same parameters, Adam slots and bf16 shadow as
    the unfused path (dE materialised, float-atomic scatter, flat Adam): differences are summation order only."""
    item_num, T, H, L, heads, B, N = cfg
    rs = np.random.RandomState(33)
    batches = []
    for _ in range(2):
        seq = _seqs(rs, B, T, N)
        seq[1, -3:] = seq[0, -1]                       # repeated ids inside the batch (several sparse rows per item)
        pos = rs.randint(1, N + 1, size=B).astype(np.int32)
        pos[2] = pos[3]                                # repeated labels
        batches.append((seq, pos))
    states = []
    for fuse in (True, False):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype=ld)
        eng.fuse_adam = fuse
        snaps = []
        for seq, pos in batches:
            eng.train_step(seq, pos, N, 5e-4, rate=0.3)
            torch.cuda.synchronize()
            sh = eng.shadow.float().cpu().numpy().copy() if eng.shadow is not None else np.zeros(1)
            snaps.append((eng.theta.cpu().numpy().copy(), eng.adam_m.cpu().numpy().copy(), eng.adam_v.cpu().numpy().copy(), sh))
        if eng.shadow is not None:                     # each engine on its own, whatever the summation order
            assert_shadow_is_bf16_of_theta(eng)
        states.append(snaps)
    (a1, a2), (b1, b2) = states
    # after ONE step from identical state the two paths differ by summation order only
    assert nerr(a1[1], b1[1]) < 2e-5 and nerr(a1[2], b1[2]) < 2e-5          # Adam m, v
    # parameters: Adam divides by sqrt(v)+eps, so an element whose gradient is ~eps (1e-8) turns last-bit differences of
    # the gradient sum into O(lr) differences of the update; everything else agrees to 2e-6
    d = np.abs(a1[0] - b1[0])
    assert np.mean(d < 2e-6) > 0.999 and d.max() < 1.1e-3
    assert np.mean(a1[3] != b1[3]) < 1e-3                                    # bf16 shadow: last-bit rounding flips only
    # the second step starts from (slightly) different parameters: ReLU branch flips of near-zero pre-activations then
    # move individual gradients by O(1e-3) (see oracle.forward_rep); require agreement at that level only
    # (which entries flip depends on the last bits of step 1: the bound is a sanity level, the equivalence proper is step 1)
    assert nerr(a2[1], b2[1]) < 3e-2 and np.abs(a2[0] - b2[0]).max() < 2.5e-3


@pytest.mark.parametrize("ld", ["bf16", "x3"])
def test_fused_update_with_a_hot_item_bucket(ld):
    """One item in 600 input positions and 120 labels of the batch (popular items / Zipf ids): its 64-id bucket takes the heavy
    path of the fused update (lists fetched 256 entries at a time, gradient rows in deep batches, more than one chunk).  One step
    from identical state against the unfused path (dE materialised, float-atomic scatter, flat Adam): summation order only."""
    item_num, T, H, L, heads, B, N = BF16_CFGS[1]
    rs = np.random.RandomState(35)
    seq = _seqs(rs, B, T, N)
    seq[:200, -3:] = 77
    seq[200:230, -1] = 78                              # a second busy id in the same bucket
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    pos[:120] = 77
    pos[120:160] = 4000                                # ... and a busy label elsewhere
    snaps = []
    for fuse in (True, False):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype=ld)
        eng.fuse_adam = fuse
        eng.train_step(seq, pos, N, 5e-4, rate=0.3)
        torch.cuda.synchronize()
        snaps.append((eng.theta.cpu().numpy().copy(), eng.adam_m.cpu().numpy().copy(), eng.adam_v.cpu().numpy().copy()))
    a, b = snaps
    assert nerr(a[1], b[1]) < 2e-5 and nerr(a[2], b[2]) < 2e-5
    d = np.abs(a[0] - b[0])
    assert np.mean(d < 2e-6) > 0.999 and d.max() < 1.1e-3
    row = slice(77 * H, 78 * H)                        # the hot row itself received every term
    assert np.abs(a[1][row]).max() > 0 and nerr(a[1][row], b[1][row]) < 2e-5


@pytest.mark.parametrize("cfg", [BF16_CFGS[0], BF16_CFGS[1]])
def test_both_bf16_update_forms_agree(cfg):
    """The two fused bf16 table updates -- k_tab16 (operand from the shadow rows, the default) and k_tab_upd (theta tile read once
    and kept in LDS) -- compute the same update from the same state: identical operand values (bf16(theta) either way), the same
    sparse lists; differences are MFMA shape / summation order only (Adam m, v 2e-5; shadow: last-bit flips)."""
    item_num, T, H, L, heads, B, N = cfg
    rs = np.random.RandomState(41)
    seq = _seqs(rs, B, T, N)
    seq[1, -3:] = seq[0, -1]
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    pos[2] = pos[3]
    out = []
    for form in ("sh", "resident"):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="bf16")
        eng.bf16_update = form
        eng.train_step(seq, pos, N, 5e-4, rate=0.3)
        torch.cuda.synchronize()
        out.append((eng.theta.cpu().numpy().copy(), eng.adam_m.cpu().numpy().copy(), eng.adam_v.cpu().numpy().copy(),
                    eng.shadow.float().cpu().numpy().copy()))
        assert_shadow_is_bf16_of_theta(eng)
    a, b = out
    assert nerr(a[1], b[1]) < 2e-5 and nerr(a[2], b[2]) < 2e-5
    d = np.abs(a[0] - b[0])
    assert np.mean(d < 2e-6) > 0.999 and d.max() < 1.1e-3
    assert np.mean(a[3] != b[3]) < 1e-3


def test_split_kd_step_matches_all_f32_kd_step():
    """Distilled step with a bf16 shadow (Engine.kd_split): train rows go through the bf16 flash logits + fused table update,
    the exemplar rows through the exact-f32 KD kernels whose table gradient enters the fused update as a dense term.  One
    step must leave the Adam state of the all-f32 KD step up to the bf16 rounding of the train rows' logit operands."""
    item_num, T, H, L, heads, B, N = BF16_CFGS[1]
    n_ex, Np = 37, 4000
    rs = np.random.RandomState(12)
    seq = _seqs(rs, B + n_ex, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    teacher = torch.from_numpy(rs.standard_normal((50, Np)).astype(np.float32)).cuda()
    trow = rs.randint(0, 50, size=n_ex).astype(np.int32)
    out = []
    for split in (True, False):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="bf16")
        eng.kd_split, eng.kd_fast = split, False
        loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3, teacher=teacher, ex_trow=trow, lambda_=0.7)
        torch.cuda.synchronize()
        out.append((float(loss.item()), eng.adam_m.cpu().numpy().copy(), eng.theta.cpu().numpy().copy()))
    (la, ma, ta), (lb, mb, tb) = out
    assert abs(la - lb) < 5e-3 * abs(lb)
    span = (item_num + 1) * H
    assert nerr(ma[:span], mb[:span]) < 3e-2              # table gradient (m = 0.1 g after one step)
    assert nerr(ma[span:], mb[span:], floor=1e-6) < 3e-2  # every other parameter
    assert np.abs(ta - tb).max() < 1.1e-3                 # one Adam step moves a parameter by at most lr


# (Np % 4 == 0: the teacher-readout kernel k_lx3r -- 4000: whole blocks; 4004: a 4-item partial block, two exemplar chunks; 648: one block
#  per range, empty ranges, a partial block alone in its range; Np % 4 != 0: unaligned teacher rows -> the round-2 readout kernel)
@pytest.mark.parametrize("cfg,n_ex,Np", [(BF16_CFGS[1], 37, 4000), (BF16_CFGS[0], 70, 650), (BF16_CFGS[1], 200, 4321),
                                         (BF16_CFGS[1], 150, 4004), (BF16_CFGS[0], 70, 648)])
def test_kd_fast_x3_step_matches_exact_oracle(cfg, n_ex, Np):
    """The all-flash distilled step at float32 grade (logits_dtype = x3): loss and the whole gradient (from Adam's first moment
    after one step, m = 0.1 g) against the plain float64 oracle of ADER.py:108-137 at the bounds of the exact-f32 kernels with
    bf16x3 block GEMMs: loss 2e-5, every gradient tensor 6e-4 normalised."""
    item_num, T, H, L, heads, B, N = cfg
    rs = np.random.RandomState(5)
    seq = _seqs(rs, B + n_ex, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    pos[0] = N
    teacher = torch.from_numpy((rs.standard_normal((n_ex + 9, Np)) * 2).astype(np.float32)).cuda()
    trow = rs.permutation(n_ex + 9)[:n_ex].astype(np.int32)
    lam = 0.7
    eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="x3")
    p64 = _params(eng, torch.float64)
    eng.global_step = 3
    loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3, teacher=teacher, ex_trow=trow, lambda_=lam)
    torch.cuda.synchronize()
    eng.check_status()
    assert eng._ws.get("lbf_pO2") is not None                     # the fast path ran
    mk = relu_masks_of(eng)
    ol, og = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=8, step=3, relu_masks=mk,
                              ex_logits=teacher.cpu()[trow.astype(np.int64)].double(), lambda_=lam)
    assert abs(float(loss.item()) - float(ol)) < 2e-5 * max(1.0, abs(float(ol)))
    for k in eng.layout:
        g = eng.view(eng.adam_m, k).cpu().numpy() / 0.1
        e = nerr(g, og[k].numpy(), floor=1e-4)
        assert e < 6e-4, (k, e)


@pytest.mark.parametrize("n_train,n_ex", [(1300, 0), (1100, 200)])
def test_more_than_1024_rows_per_step_on_the_flash_path(n_train, n_ex):
    """Steps with more than 1024 rows (reference --batch_size is free, main.py:94): the flash logit kernels work on 128-row chunks and
    the fused update loops over the batch, so logits_dtype bf16 / x3 take up to Engine.MAX_ROWS_FAST rows (the exact-f32 logit
    kernels keep per-row state in LDS: 1024, asserted).  x3 step, vanilla and distilled, against the float64 oracle at the bounds
    of test_kd_fast_x3_step_matches_exact_oracle."""
    item_num, T, H, L, heads, N, Np = 1500, 50, 150, 2, 1, 1400, 1200
    rs = np.random.RandomState(6)
    seq = _seqs(rs, n_train + n_ex, T, N)
    pos = rs.randint(1, N + 1, size=n_train).astype(np.int32)
    eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="x3")
    p64 = _params(eng, torch.float64)
    eng.global_step = 2
    kw, okw = {}, {}
    if n_ex:
        teacher = torch.from_numpy((rs.standard_normal((n_ex, Np)) * 2).astype(np.float32)).cuda()
        kw = dict(teacher=teacher, ex_trow=np.arange(n_ex, dtype=np.int32), lambda_=0.7)
        okw = dict(ex_logits=teacher.cpu().double(), lambda_=0.7)
    loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3, **kw)
    torch.cuda.synchronize()
    eng.check_status()
    mk = relu_masks_of(eng)
    ol, og = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=8, step=2, relu_masks=mk, **okw)
    assert abs(float(loss.item()) - float(ol)) < 2e-5 * max(1.0, abs(float(ol)))
    for k in eng.layout:
        g = eng.view(eng.adam_m, k).cpu().numpy() / 0.1
        e = nerr(g, og[k].numpy(), floor=1e-4)
        assert e < 6e-4, (k, e)
    with pytest.raises(RuntimeError):              # the exact-f32 logit kernels: loud limit, no silent truncation
        _engine(item_num, T, H, L, heads, seed=8, logits_dtype="f32").train_step(seq, pos, N, 5e-4, rate=0.3, **kw)


@pytest.mark.parametrize("cfg,n_ex,Np", [(BF16_CFGS[1], 37, 4000), (BF16_CFGS[0], 70, 650), (BF16_CFGS[1], 200, 4321)])
def test_kd_fast_step_matches_bf16_aware_oracle(cfg, n_ex, Np):
    """Distilled step with every row on the bf16 flash path (Engine.kd_fast: exemplar rows as their own chunks with the softmax
    over the first Np items, teacher readout in the forward, teacher term subtracted inside the fused table update).  One step
    from zero Adam state leaves m = 0.1 g, so the whole gradient is read back from the optimiser state and compared with the
    oracle evaluated with the same bf16 operand rounding of the logits product (reference: ADER.py:108-137): loss 3e-4, every
    gradient tensor 6e-3 normalised (as test_bf16_logits_path_matches_bf16_aware_oracle)."""
    item_num, T, H, L, heads, B, N = cfg
    rs = np.random.RandomState(5)
    seq = _seqs(rs, B + n_ex, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    pos[0] = N
    teacher = torch.from_numpy((rs.standard_normal((n_ex + 9, Np)) * 2).astype(np.float32)).cuda()
    trow = rs.permutation(n_ex + 9)[:n_ex].astype(np.int32)
    lam = 0.7
    eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="bf16")
    assert eng.kd_fast
    p64 = _params(eng, torch.float64)
    eng.global_step = 3
    loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3, teacher=teacher, ex_trow=trow, lambda_=lam)
    torch.cuda.synchronize()
    eng.check_status()
    assert eng._ws.get("lbf_pO2") is not None                     # the fast path ran (teacher readout scratch exists)
    mk = relu_masks_of(eng)
    ol, og = R.loss_and_grads(p64, seq, pos, N, L, heads, training=True, rate=0.3, seed=8, step=3, logits_bf16=True, relu_masks=mk,
                              ex_logits=teacher.cpu()[trow.astype(np.int64)].double(), lambda_=lam)
    assert abs(float(loss.item()) - float(ol)) < 3e-4 * max(1.0, abs(float(ol)))
    for k in eng.layout:
        g = eng.view(eng.adam_m, k).cpu().numpy() / 0.1            # m = (1 - beta1) g after the first update of a zero state
        e = nerr(g, og[k].numpy(), floor=1e-4)
        assert e < 6e-3, (k, e)


def test_kd_fast_equals_split_kd():
    """The all-flash distilled step against the split one (exemplar rows on the exact-f32 KD kernels): same Adam state up to the
    bf16 rounding of the exemplar rows' logit operands."""
    item_num, T, H, L, heads, B, N = BF16_CFGS[1]
    n_ex, Np = 37, 4000
    rs = np.random.RandomState(12)
    seq = _seqs(rs, B + n_ex, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    teacher = torch.from_numpy(rs.standard_normal((50, Np)).astype(np.float32)).cuda()
    trow = rs.randint(0, 50, size=n_ex).astype(np.int32)
    out = []
    for fast in (True, False):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype="bf16")
        eng.kd_fast = fast
        loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3, teacher=teacher, ex_trow=trow, lambda_=0.7)
        torch.cuda.synchronize()
        out.append((float(loss.item()), eng.adam_m.cpu().numpy().copy(), eng.theta.cpu().numpy().copy()))
    (la, ma, ta), (lb, mb, tb) = out
    assert abs(la - lb) < 5e-3 * abs(lb)
    span = (item_num + 1) * H
    assert nerr(ma[:span], mb[:span]) < 3e-2
    assert nerr(ma[span:], mb[span:], floor=1e-6) < 3e-2
    assert np.abs(ta - tb).max() < 1.1e-3


@pytest.mark.parametrize("ld,variant", [("bf16", "fused"), ("x3", "fused"), ("f32", "unfused"), ("x3", "unfused"), ("x3", "ewc"),
                                        ("f32", "ewc")])
def test_train_step_is_bitwise_reproducible(ld, variant):
    """Determinism (SURVEY 8b "no float atomics on the parity path"; the reference sets TF_DETERMINISTIC_OPS, main.py:121-122):
    two engines stepping the same batches from the same state end bit-identical -- on the default path (one-launch forward,
    session-tiled backward, batched weight gradients, id-sorted sparse lists, fused table update on two streams) AND on the unfused
    one (exact-f32 logits, or the fused update switched off, or the EWC baseline whose penalty lives in the dense gradient buffer,
    EWC.py:115-124): its input-embedding rows are added in position order from the bucketed lists and its one-hot rows by a single
    writer per table row (rounds 1-3: float atomicAdd scatters, last bits differed from run to run)."""
    item_num, T, H, L, heads, B, N = BF16_CFGS[1]
    rs = np.random.RandomState(77)
    batches = []
    for _ in range(3):
        seq = _seqs(rs, B, T, N)
        seq[1, -4:] = seq[0, -1]                       # repeated ids: several sparse rows per table row
        seq[2, -1] = seq[0, -1]
        pos = rs.randint(1, N + 1, size=B).astype(np.int32)
        pos[5] = pos[6]
        pos[9] = pos[6]
        batches.append((seq, pos))
    finals = []
    for _ in range(2):
        eng = _engine(item_num, T, H, L, heads, seed=8, logits_dtype=ld)
        if variant == "unfused":
            eng.fuse_adam = False
        elif variant == "ewc":
            eng.ewc_snapshot()
            eng.compute_fisher(batches[0][0][:6], batches[0][1][:6], N)
            eng.ewc["lam"] = 50.0
            eng.param("emb").mul_(1.01)                # away from the snapshot: a non-zero penalty
            eng.refresh_shadow()
        for seq, pos in batches:
            eng.train_step(seq, pos, N, 5e-4, rate=0.3)
        torch.cuda.synchronize()
        sh = eng.shadow.clone() if eng.shadow is not None else torch.zeros(1)
        if eng.shadow is not None:
            assert_shadow_is_bf16_of_theta(eng)
        finals.append((eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), sh, float(eng.loss.item())))
    for x, y in zip(finals[0][:4], finals[1][:4]):
        assert torch.equal(x, y)
    assert finals[0][4] == finals[1][4]


def test_adam_keeps_bf16_shadow_in_sync():
    eng = _engine(301, 20, 64, 1, 2, logits_dtype="bf16")          # odd row count: float4 groups straddle table rows
    g = torch.Generator().manual_seed(9)
    for it in range(2):
        eng.grad.copy_(torch.randn(eng.P, generator=g) * 0.01)
        eng.adam(5e-4)
    torch.cuda.synchronize()
    sh = eng.shadow.view(-1, 168)[:eng.V].float().cpu()
    emb = eng.param("emb").cpu()
    assert torch.equal(sh[:, :64], emb.bfloat16().float())
    assert torch.all(sh[:, 64:] == 0)


def test_adam_matches_tf_formula():
    eng = _engine(300, 20, 64, 1, 2)
    p0 = _params(eng, torch.float32)
    g = torch.Generator().manual_seed(5)
    grads = {k: torch.randn(v.shape, generator=g) * 0.01 for k, v in p0.items()}
    opt = R.TFAdam(p0)
    for it in range(3):
        for k in eng.layout:
            eng.gradient(k).copy_(grads[k] * (it + 1))
        eng.adam(5e-4)
        opt.step(p0, {k: v * (it + 1) for k, v in grads.items()}, 5e-4)
    torch.cuda.synchronize()
    for k in eng.layout:
        assert nerr(eng.param(k).cpu(), p0[k]) < 2e-6, k
    assert eng.global_step == 3


def test_three_train_steps_track_the_oracle():
    item_num, T, H, L, heads, B, N = CFGS[0]
    eng = _engine(item_num, T, H, L, heads, seed=7)
    params = _params(eng, torch.float32)
    opt = R.TFAdam(params)
    rs = np.random.RandomState(4)
    for it in range(3):
        seq = _seqs(rs, B, T, N)
        pos = rs.randint(1, N + 1, size=B).astype(np.int32)
        loss = eng.train_step(seq, pos, N, 5e-4, rate=0.3)
        ol = R.train_step(params, opt, seq, pos, N, L, heads, 5e-4, training=True, rate=0.3, seed=7, step=it)
        assert abs(float(loss.item()) - ol) < 1e-4 * max(1.0, abs(ol))
    for k in eng.layout:
        # Adam normalises tiny gradients to +-lr, so compare on the scale of the accumulated update (3*lr)
        d = np.abs(eng.param(k).cpu().numpy() - params[k].numpy()).max()
        assert d < 3e-4, (k, d)


@pytest.mark.parametrize("cfg", CFGS)
def test_rank_is_exact_wrt_device_logits_and_matches_oracle(cfg):
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(6)
    seq = _seqs(rs, B, T, N)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    # make exact ties: duplicate a few table rows
    emb = eng.param("emb")
    emb[5] = emb[17]
    emb[40] = emb[41]
    pos[0], pos[1] = 17, 41
    ranks = eng.rank_targets(seq, pos, N)
    lg = eng.logits(seq, N).cpu().numpy()
    exp = np.array([R.rank_of_target(lg[b], int(pos[b])) for b in range(B)])
    assert np.array_equal(ranks, exp)                                    # bit-exact index work
    oracle = R.rank_all(_params(eng, torch.float32), seq, N, L, heads).numpy()
    agree = np.mean([oracle[b, pos[b] - 1] == ranks[b] for b in range(B)])
    assert agree > 0.97                                                   # float32 near-ties may swap neighbours
    olg = R.logits_from_rep(_params(eng, torch.float64), R.forward_rep(_params(eng, torch.float64), seq, L, heads), N)
    assert nerr(lg, olg.detach().numpy()) < 1e-4


@pytest.mark.parametrize("n_sp,n_tg,N", [(25600, 512, 1_000_000), (19950, 399, 43105), (7, 1, 5), (51200, 1024, 777), (1, 1, 64),
                                         (3000, 0, 65), (204800, 4096, 1_000_000)])
def test_sparse_lists_are_bucketed_in_position_order(n_sp, n_tg, N):
    """ader_sparse_lists (index work, bit-exact): entries in id order and, for one id, in position order -- i.e. a stable sort
    by id (hence grouped by 64-id bucket) -- with the bucket offsets, against numpy.  Pads (id 0), heavy duplicates, ids in the
    last bucket, and the gathered list sizes of an 8-rank data-parallel step."""
    from ader_amd._lib import call, ptr
    rs = np.random.RandomState(n_sp + N)
    seq = rs.randint(0, N + 1, size=n_sp).astype(np.int32)
    seq[rs.rand(n_sp) < 0.3] = 0
    if n_sp > 10:
        seq[:5] = N
        seq[5:9] = 1
        seq[9:200:3] = min(N, 37)                     # a hot item
    lab = rs.randint(1, N + 1, size=n_tg).astype(np.int32)
    dev = torch.device("cuda")
    d_seq, d_lab = torch.from_numpy(seq).to(dev), torch.from_numpy(lab).to(dev)
    nb1 = call("ader_sparse_lists_starts", N)
    i32 = dict(dtype=torch.int32, device=dev)
    ids, rows, st = torch.empty(n_sp, **i32), torch.empty(n_sp, **i32), torch.empty(nb1, **i32)
    tids, trows, tst = torch.empty(max(n_tg, 1), **i32), torch.empty(max(n_tg, 1), **i32), torch.empty(nb1, **i32)
    scratch = torch.empty(call("ader_sparse_lists_scratch_n", n_sp, n_tg, N), **i32)
    for rep in range(2):                              # twice: the result does not depend on the atomics' arrival order
        call("ader_sparse_lists", ptr(d_seq), n_sp, ptr(d_lab), n_tg, N, ptr(scratch), ptr(ids), ptr(rows), ptr(st), ptr(tids),
             ptr(trows), ptr(tst), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        bounds = np.arange(1, N + 64 + 1, 64)
        assert len(bounds) == nb1
        for src, got_ids, got_rows, got_st, n in ((seq, ids, rows, st, n_sp), (lab, tids, trows, tst, n_tg)):
            real = np.flatnonzero(src > 0)               # padding entries (id 0) are left out of the lists
            o = real[np.argsort(src[real], kind="stable")]
            nr = len(real)
            assert np.array_equal(got_rows.cpu().numpy()[:nr], o.astype(np.int32))
            assert np.array_equal(got_ids.cpu().numpy()[:nr], src[o])
            assert np.array_equal(got_st.cpu().numpy(), np.searchsorted(np.sort(src[src > 0]), bounds).astype(np.int32))
    # ader_sparse_lists_meta: the same lists plus the per-tile records of the update kernels -- as ONE launch on small problems
    # (every case here except the 1M-item catalogs), as ader_sparse_lists + ader_tab_tile_meta otherwise: identical outputs
    nm = call("ader_tab_meta_ints", N)
    meta_a, meta_b = torch.full((nm,), -7, **i32), torch.full((nm,), -9, **i32)
    call("ader_tab_tile_meta", ptr(ids), ptr(rows), ptr(st), ptr(tids), ptr(trows), ptr(tst), N, ptr(meta_a),
         torch.cuda.current_stream().cuda_stream)
    ids2, rows2, st2 = torch.full((n_sp,), -1, **i32), torch.full((n_sp,), -1, **i32), torch.full((nb1,), -1, **i32)
    tids2, trows2, tst2 = torch.full((max(n_tg, 1),), -1, **i32), torch.full((max(n_tg, 1),), -1, **i32), torch.full((nb1,), -1, **i32)
    scratch2 = torch.empty(call("ader_sparse_lists_scratch_n", n_sp, n_tg, N), **i32)
    for rep in range(2):
        call("ader_sparse_lists_meta", ptr(d_seq), n_sp, ptr(d_lab), n_tg, N, ptr(scratch2), ptr(ids2), ptr(rows2), ptr(st2), ptr(tids2),
             ptr(trows2), ptr(tst2), ptr(meta_b), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        nr0, nr1 = int((seq > 0).sum()), int((lab > 0).sum())
        assert torch.equal(ids2[:nr0], ids[:nr0]) and torch.equal(rows2[:nr0], rows[:nr0]) and torch.equal(st2, st)
        assert torch.equal(tids2[:nr1], tids[:nr1]) and torch.equal(trows2[:nr1], trows[:nr1]) and torch.equal(tst2, tst)
        assert torch.equal(meta_a, meta_b)


def test_herding_bit_exact_against_oracle(golden_dir):
    from make_golden import herding_inputs
    from ader_amd.exemplar import herding_max_steps
    from ader_amd import _lib
    cases = json.load(open(os.path.join(golden_dir, "herding.json")))["cases"]
    reps, offs, quota = [], [0], []
    for c in cases:
        reps.append(herding_inputs(c["seed"], c["n"], c["H"], c["dup"]))
        offs.append(offs[-1] + c["n"])
        quota.append(min(c["m"], c["n"]))
    # ... plus the size classes of the register-resident kernel (csrc/herding.hip: one wave up to 64 rows, one workgroup up to 512,
    # then 240 LDS-resident candidates, then streamed ones) at their boundaries, duplicates included -- checked against the oracle only
    cases = [dict(c) for c in cases]
    for i, (nn, mm, dup) in enumerate([(64, 64, False), (65, 30, False), (129, 129, True), (511, 40, False), (512, 512, False),
                                       (513, 77, True), (752, 90, False), (753, 753, False), (1300, 25, True), (2, 0, False)]):
        cases.append({"seed": 900 + i, "n": nn, "H": 150, "m": mm, "dup": dup, "class": "oracle-only"})
        reps.append(herding_inputs(900 + i, nn, 150, dup))
        offs.append(offs[-1] + nn)
        quota.append(min(mm, nn))
    rep = torch.from_numpy(np.concatenate(reps)).cuda()
    n, G, H = rep.shape[0], len(cases), 150
    dev = rep.device
    seg = torch.tensor(offs, dtype=torch.int64, device=dev)
    q = torch.tensor(quota, dtype=torch.int32, device=dev)
    ms = torch.tensor([herding_max_steps(m) for m in quota], dtype=torch.int32, device=dev)
    out = {}
    for fn in ("ader_herding_select", "ader_herding_select_generic"):
        D = torch.full((n * H + G + 64,), float("nan"), device=dev)
        chosen = torch.empty(n, dtype=torch.uint8, device=dev)
        sel = torch.zeros(n, dtype=torch.int32, device=dev)
        cnt = torch.full((G,), -1, dtype=torch.int32, device=dev)
        steps = torch.full((G,), -1, dtype=torch.int32, device=dev)
        _lib.call(fn, rep.data_ptr(), seg.data_ptr(), q.data_ptr(), ms.data_ptr(), G, n, H, D.data_ptr(),
                  chosen.data_ptr(), sel.data_ptr(), cnt.data_ptr(), steps.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out[fn] = (sel.cpu().numpy(), cnt.cpu().numpy(), steps.cpu().numpy())
    sel, cnt, steps = out["ader_herding_select"]
    n_ref_exact = 0
    for g, c in enumerate(cases):
        o_sel, o_steps = herding_ref.herding_select(reps[g], c["m"])
        for fn, (sel_, cnt_, steps_) in out.items():
            got = sel_[offs[g]:offs[g] + cnt_[g]].tolist()
            assert got == o_sel, (fn, c["n"], c["m"], c["dup"])          # HIP == canonical spec, every case, both kernels
            assert steps_[g] == o_steps, (fn, c["n"], c["m"])
        if c["class"] == "exact":
            assert sel[offs[g]:offs[g] + cnt[g]].tolist() == c["selected"]    # == the reference's own herding()
            n_ref_exact += 1
    assert n_ref_exact >= 30


def test_edge_cases_single_row_and_short_catalog():
    eng = _engine(100, 50, 150, 2, 1)
    seq = np.zeros((1, 50), dtype=np.int32)
    seq[0, -1] = 3
    pos = np.array([7], dtype=np.int32)
    loss = eng.loss_and_grad(seq, pos, 11, rate=0.0)
    torch.cuda.synchronize()
    ol, og = R.loss_and_grads(_params(eng, torch.float64), seq, pos, 11, 2, 1, training=True, rate=0.0)
    assert abs(float(loss.item()) - float(ol)) < 2e-5
    for k in ("emb", "pos", "b0.wq", "b1.w2", "lnf_g"):
        assert nerr(eng.gradient(k).cpu().numpy(), og[k].numpy(), floor=1e-4) < 3e-4, k
    with pytest.raises(Exception):
        bad = seq.copy()
        bad[0, -1] = 101 + 5                     # id outside the table: must be reported, never clamped silently
        eng.forward(eng._dev_i32(bad))
        torch.cuda.synchronize()
        eng.check_status()
