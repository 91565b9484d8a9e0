"""Evaluation ranking on the bf16 matrix cores (Engine.rank_targets(dtype="x3"), ader_rank_targets_x3): an x3 filter that decides the
(row, item) pairs whose logit is provably above / below the row's target logit, an exact-f32 recheck of the rest, the exact kernel when the
candidate list overflows.  The contract is an equality, ties included: ranks(x3) == ranks(f32) on every input."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _engine(item_num, T, H, L, heads, seed=0, **kw):
    from ader_amd.engine import Engine
    kw.setdefault("logits_dtype", "f32")
    eng = Engine(item_num, maxlen=T, hidden_units=H, num_blocks=L, num_heads=heads, seed=seed, **kw)
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


def _seqs(rs, B, T, n_items, full=False):
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = T if full else int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, n_items + 1, size=ln)
    return seq


# item_num, T, H, L, heads, B, N: H mod 8 = 6, 0, 4; B below / at / over one and two 128-row chunks; N no multiple of 32, below one
# block, smaller than the 8 item ranges (some are empty)
SHAPES = [(700, 50, 150, 2, 1, 70, 650), (300, 20, 64, 1, 2, 9, 300), (1000, 50, 150, 2, 3, 130, 777),
          (64, 8, 12, 1, 1, 3, 33), (64, 8, 12, 1, 1, 1, 31), (2000, 20, 150, 1, 1, 257, 1999)]


def _case(cfg, seed=6):
    item_num, T, H, L, heads, B, N = cfg
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(seed)
    return eng, _seqs(rs, B, T, N), rs.randint(1, N + 1, size=B).astype(np.int32), N


def _plant_ties(eng, pos, N):
    """Rows equal to a target's row below and above its index (exact ties, as the f32 rank test plants them) and rows one ulp away in one
    channel, up and down (near-ties).  Returns the number of planted rows; each is a candidate for at least the row of its target."""
    emb = eng.param("emb")
    pos[0], pos[1] = 17, 41
    emb[5] = emb[17]
    emb[N - 3] = emb[17]
    emb[40] = emb[41]
    emb[N - 5] = emb[41]
    for dst, src, ch, up in ((60, 17, 3, True), (61, 17, 3, False), (N - 7, 41, 0, True), (N - 8, 41, 7, False)):
        row = emb[src].clone()
        row[ch] = torch.nextafter(row[ch], torch.tensor(float("inf") if up else float("-inf"), device=row.device))
        emb[dst] = row
    return 8


@pytest.mark.parametrize("cfg", SHAPES)
def test_x3_ranks_equal_f32_ranks(cfg):
    eng, seq, pos, N = _case(cfg)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3")
    print("stats", eng.last_rank_stats)
    assert np.array_equal(got, ref)
    assert eng.last_rank_stats["pairs"] == cfg[5] * N


@pytest.mark.parametrize("cfg", [SHAPES[0], SHAPES[2]])
def test_exact_ties_and_near_ties(cfg):
    eng, seq, pos, N = _case(cfg)
    planted = _plant_ties(eng, pos, N)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3")
    print("stats", eng.last_rank_stats)
    assert np.array_equal(got, ref)
    assert eng.last_rank_stats["candidates"] >= planted          # the recheck path ran
    assert eng.last_rank_stats["overflowed_chunks"] == 0


def test_integer_operands_match_int64_count():
    import ader_amd.ops  # noqa: F401
    B, N, H = 130, 777, 150
    rs = np.random.RandomState(3)
    rep = rs.randint(-3, 4, size=(B, H)).astype(np.float32)
    emb = rs.randint(-3, 4, size=(N + 1, H)).astype(np.float32)
    tgt = rs.randint(1, N + 1, size=B).astype(np.int32)
    dev = torch.device("cuda")
    got = torch.ops.ader.rank_of_target_x3(torch.from_numpy(rep).to(dev), torch.from_numpy(emb).to(dev), torch.from_numpy(tgt).to(dev), N)
    s = rep.astype(np.int64) @ emb[1:].astype(np.int64).T                       # [B, N], exact
    tl = s[np.arange(B), tgt - 1][:, None]
    n = np.arange(N)[None, :]
    exp = ((s > tl) | ((s == tl) & (n < (tgt - 1)[:, None]))).sum(1)
    assert np.array_equal(got.cpu().numpy(), exp.astype(np.int32))
    ref = torch.ops.ader.rank_of_target(torch.from_numpy(rep).to(dev), torch.from_numpy(emb).to(dev), torch.from_numpy(tgt).to(dev), N)
    assert np.array_equal(ref.cpu().numpy(), exp.astype(np.int32))


def test_overflowing_candidate_list_falls_back():
    eng, seq, pos, N = _case(SHAPES[2])
    _plant_ties(eng, pos, N)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3", cand_cap=4)
    assert eng.last_rank_stats["overflowed_chunks"] >= 1
    assert np.array_equal(got, ref)


def test_fallback_ranks_on_the_same_session_forward():
    """Short sessions from the host (sparse: "auto" packs them) over two chunks with a tiny list: the chunks that fall back must be
    ranked on the forward the f32 call uses for a host batch, not on the one a device slice would get."""
    item_num, T, H, L, heads, _, N = SHAPES[2]
    eng = _engine(item_num, T, H, L, heads)
    rs = np.random.RandomState(12)
    B = eng.MAX_ROWS + 70
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, 6))
        seq[b, T - ln:] = rs.randint(1, N + 1, size=ln)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3", cand_cap=4)
    assert eng.last_rank_stats["overflowed_chunks"] == 2
    assert np.array_equal(got, ref)
    assert np.array_equal(eng.rank_targets(seq, pos, N, dtype="x3"), ref)


@pytest.mark.parametrize("cfg", [SHAPES[0], SHAPES[2], SHAPES[5]])
def test_filter_filters_and_bound_has_margin(cfg):
    """A kernel that sends everything to the recheck cannot pass: <= 1 % of the pairs are candidates (expected for Gaussian-like operands:
    2 KAPPA sqrt(H) / sqrt(2 pi) ~ 1.2e-3 -- derived, an eight-fold margin), no overflow at the default cap; and the observed
    |s_x3 - s_f32| / delta stays within the derivation's 2^-14.1 / 2^-13 = 0.47 <= 0.5."""
    eng, seq, pos, N = _case(cfg)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3")
    st = eng.last_rank_stats
    print("candidate share %.3e  max_err_over_delta %.4f  %r" % (st["candidates"] / st["pairs"], st["max_err_over_delta"], st))
    assert np.array_equal(got, ref)
    assert st["candidates"] <= 0.01 * st["pairs"]
    assert st["overflowed_chunks"] == 0
    if st["candidates"] > 0:
        assert st["max_err_over_delta"] <= 0.5


def test_larger_randomized_run_with_outlier_norms():
    """B = 512, N = 20,011, H = 150, one block; table-row norms spread over two decades, so Emax is set by an outlier."""
    item_num, T, H, B, N = 20100, 20, 150, 512, 20011
    eng = _engine(item_num, T, H, 1, 1)
    g = torch.Generator().manual_seed(5)
    scale = 10.0 ** (torch.rand(item_num + 1, generator=g) * 2.0 - 2.0)          # 0.01 .. 1
    emb = eng.param("emb")
    scale[123] = 3.0                                                              # the outlier that sets Emax
    emb.mul_(scale.to(emb.device)[:, None])
    rs = np.random.RandomState(8)
    seq, pos = _seqs(rs, B, T, N), rs.randint(1, N + 1, size=B).astype(np.int32)
    ref = eng.rank_targets(seq, pos, N, dtype="f32")
    got = eng.rank_targets(seq, pos, N, dtype="x3")
    print("stats", eng.last_rank_stats)       # (the band scales with Emax: small-norm rows crowd it, chunks may take the fallback)
    assert np.array_equal(got, ref)


def test_engine_setting_and_unsupported_hidden_size():
    """rank_dtype of the engine is what dtype=None takes; a hidden size outside k_lx3k's takes the exact kernel silently."""
    eng, seq, pos, N = _case(SHAPES[1])
    eng.rank_dtype = "x3"
    eng.last_rank_stats = None
    got = eng.rank_targets(seq, pos, N)
    assert eng.last_rank_stats is not None and np.array_equal(got, eng.rank_targets(seq, pos, N, dtype="f32"))
    e10 = _engine(64, 8, 10, 1, 1, rank_dtype="x3")                              # H mod 8 = 2
    rs = np.random.RandomState(1)
    s10, p10 = _seqs(rs, 5, 8, 33), rs.randint(1, 34, size=5).astype(np.int32)
    assert np.array_equal(e10.rank_targets(s10, p10, 33), e10.rank_targets(s10, p10, 33, dtype="f32"))
    assert e10.last_rank_stats is None
    with pytest.raises(RuntimeError):
        eng.rank_targets(seq, pos, N, dtype="bf16")


def test_driver_surface_evaluator_results_identical():
    """Evaluator over a synthetic session list with model.Ader(rank_dtype="x3") and ("f32") from the same seed: identical ranks, metrics."""
    import random

    from ader_amd.data import Evaluator
    from ader_amd.main import build_parser
    from ader_amd.model import Ader
    item_num, N = 300, 280
    rs = np.random.RandomState(4)
    sessions = [[int(x) for x in rs.randint(1, N + 1, size=int(rs.randint(2, 12)))] for _ in range(150)]
    out = []
    for rd in ("x3", "f32"):
        args = build_parser().parse_args(["--rank_dtype", rd, "--hidden_units", "64", "--maxlen", "20", "--num_blocks", "1"])
        assert args.rank_dtype == rd
        model = Ader(item_num, args)
        assert model.engine.rank_dtype == rd
        random.seed(9)
        ev = Evaluator(sessions, False, args.maxlen, 64, N, "test", model, None)       # whole sessions: every prefix is a row (util.py:276-350)
        ev.evaluate(1)
        out.append((list(ev.ranks), ev.results()))
        if rd == "x3":
            assert model.engine.last_rank_stats is not None and model.engine.last_rank_stats["pairs"] == len(ev.ranks) * N
    assert len(out[0][0]) > 150 and out[0] == out[1]
