"""Host side of the x3 evaluation ranking (no GPU): the export, the options, and the error bound of the filter emulated on the CPU."""
import inspect

import numpy as np
import pytest
import torch


def test_symbols_and_options():
    from ader_amd import _lib
    from ader_amd.engine import Engine
    from ader_amd.engine import infer
    from ader_amd.main import _BUILD_FLAGS, build_parser
    assert "ader_rank_targets_x3" in _lib.exported_symbols() and "ader_rank_emax" in _lib.exported_symbols()
    flag = [f for f in _BUILD_FLAGS if f[0] == "rank_dtype"]
    assert len(flag) == 1 and flag[0][1] == "f32" and flag[0][3] == ("f32", "x3")
    args = build_parser().parse_args([])
    assert args.rank_dtype == "f32"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--rank_dtype", "bf16"])
    sig = inspect.signature(Engine.__init__)
    assert sig.parameters["rank_dtype"].default == "f32"
    rt = inspect.signature(Engine.rank_targets)
    assert rt.parameters["dtype"].default is None and rt.parameters["cand_cap"].default is None
    with pytest.raises(RuntimeError, match="rank_dtype"):        # validated before anything touches the GPU
        Engine(100, rank_dtype="bf16")
    assert infer.RANK_X3_KAPPA == 2.0 ** -13
    # the hidden sizes of k_lx3k (lx3f_supports): even, 8 <= H <= 160, H mod 8 in {0, 4, 6}
    assert [h for h in range(1, 170) if infer.rank_x3_supports(h)] == [h for h in range(8, 161, 2) if h % 8 != 2]


def _split(x):
    """hi = bf16(x), lo = bf16(x - hi), round-to-nearest-even, as k_lx3_prep and the block staging cut their operands."""
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _dots(r, e):
    """(s_x3, s_32, s_64) of r [B,H] . e [N,H]: the three-term products accumulated in float32 in k order (lo.hi, hi.lo, hi.hi per
    k, the kernel's order of terms; products of two bf16 values are exact in float32), the float32 fma-like chain, and float64."""
    rh, rl = _split(r)
    eh, el = _split(e)
    s3 = torch.zeros(r.shape[0], e.shape[0], dtype=torch.float32)
    s32 = torch.zeros_like(s3)
    for k in range(r.shape[1]):
        s3 = s3 + el[None, :, k] * rh[:, None, k]
        s3 = s3 + eh[None, :, k] * rl[:, None, k]
        s3 = s3 + eh[None, :, k] * rh[:, None, k]
        s32 = (s32.double() + e[None, :, k].double() * r[:, None, k].double()).float()       # one rounding per step: an fma
    s64 = r.double() @ e.double().T
    return s3.double(), s32.double(), s64


def _operands(kind, H, rs):
    B, N = 24, 96
    if kind == "random":
        r = rs.standard_normal((B, H)) * np.exp(rs.uniform(-3, 3, size=(B, 1)))
        e = rs.standard_normal((N, H)) * np.exp(rs.uniform(-3, 3, size=(N, 1)))
    else:
        # adversarial: every entry positive (no cancellation in the sum: sum |r||e| = the sum itself, and r parallel-ish to e makes
        # Cauchy-Schwarz nearly tight), mantissas where the two-term bf16 split leaves its largest residual: x = m (1 + 2^-8 + 2^-16 +
        # a few low bits), just above the rounding ties of both cuts
        base = 1.0 + 2.0 ** -8 + 2.0 ** -16 + rs.randint(1, 128, size=(B + N, H)) * 2.0 ** -23
        x = base * 2.0 ** rs.randint(-1, 1, size=(B + N, 1))
        r, e = x[:B], x[B:]
    return torch.from_numpy(r.astype(np.float32)), torch.from_numpy(e.astype(np.float32))


@pytest.mark.parametrize("H", [12, 64, 150])
@pytest.mark.parametrize("kind", ["random", "adversarial"])
def test_x3_error_is_within_half_the_band(kind, H):
    from ader_amd.engine.infer import RANK_X3_KAPPA
    r, e = _operands(kind, H, np.random.RandomState(H + len(kind)))
    s3, s32, s64 = _dots(r, e)
    err = (s3 - s64).abs() + (s32 - s64).abs()
    bound = 0.5 * RANK_X3_KAPPA * r.double().norm(dim=1)[:, None] * e.double().norm(dim=1)[None, :]
    worst = float((err / bound).max())
    print("%s H=%d: worst (|s_x3 - s_64| + |s_32 - s_64|) / (0.5 KAPPA |r||e|) = %.4f" % (kind, H, worst))
    assert bool((err <= bound).all())
