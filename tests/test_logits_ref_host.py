"""Self-checks of oracle/logits_ref.py, the element-wise float64 anchor behind tests/test_gpu_logits_anchor.py (CPU only).  The
emulation of k_logits_tile<MODE_STORE> and of k_row_lse must pass its own check on every operand family, and check_store /
check_row_lse must reject every planted fault, naming a (row, item) inside the faulted region with its chunk and tile:
  (a) the last k step dropped, at H = 150 (its two real columns) and at H = 157 (its one);
  (b) the rows of chunk 1 computed from row b ^ 64;
  (c) the columns of the last partial tile shifted by one item;
  (d) one operand rounded to bf16;
  (e) ONE element off by 64 ulps of its measure at the smallest |logit| of the tensor -- which the tensor-wide criterion that held
      Engine.logits before (nerr < 1e-4 of the largest logit, tests/test_gpu_parity.py) accepts;
  row_lse: the maximum taken over ncols - 1 columns, and thread 255's partial sum dropped.
The fault of the maximum needs a dominant entry beyond float32's exp range above the rest (+100 here): log-sum-exp does not depend on
the shift, so a maximum that misses the entry is wrong only when expf(x - m) overflows (x - m > 88.7)."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import logits_ref as G
from oracle import x3_step_ref as X

SHAPES = {"H150": (130, 650, 150), "H157": (130, 650, 157), "H1": (65, 65, 1), "H160": (65, 129, 160)}     # B, N, H


@functools.lru_cache(maxsize=None)
def _built(name):
    """(rep, E, N, reference, emulation) of a shape: computed once, shared, never modified."""
    B, N, H = SHAPES[name]
    rep, E = G.operands(B, N, H, seed=5)
    return rep, E, N, G.reference(rep, E, N), G.emulate(rep, E, N)


def _nerr(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max())


def _rejects(name, fault):
    rep, E, N, ref, emu = _built(name)
    dev, (r0, r1, i0, i1) = G.plant(fault, rep, E, N, emu=emu, ref=ref)
    with pytest.raises(X.ParityError) as ei:
        G.check_store(dev, rep, E, N, ref=ref, emu=emu)
    found = re.search(r"worst \(row (\d+), item (\d+)\) chunk (\d+) tile (\d+)", str(ei.value))
    assert found, str(ei.value)
    b, it, chunk, tile = (int(v) for v in found.groups())
    assert r0 <= b <= r1 and i0 <= it <= i1, str(ei.value)
    assert chunk == b // 64 and tile == (it - 1) // 64
    return dev


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_emulation_passes_its_own_check(name):
    rep, E, N, ref, emu = _built(name)
    err, base, bound = G.check_store(emu.clone(), rep, E, N, ref=ref, emu=emu)
    assert err == base and bound >= X.FLOOR
    assert base < 2.0 ** -20, base                          # float32 grade in the term-sum measure: nothing of order one
    assert tuple(emu.shape) == (SHAPES[name][0], N) and emu.dtype == torch.float32


def test_reference_is_the_plain_product_and_its_term_sum():
    rep, E, N, (s, t), _ = _built("H150")
    b, n = 77, 640
    terms = rep[b].double() * E[n + 1].double()
    assert abs(float(s[b, n]) - float(terms.sum())) < 1e-12 and abs(float(t[b, n]) - float(terms.abs().sum())) < 1e-12
    assert bool((t >= s.abs()).all())


def test_emulation_is_the_fmaf_chain_in_k_order():
    """One element by hand: acc = fmaf(rep[b, k], E[n, k], acc) for k = 0 .. H - 1 (the float64 product of two float32 is exact)."""
    rep, E, N, _, emu = _built("H150")
    for b, n in ((0, 0), (129, 649), (64, 640)):
        acc = np.float32(0.0)
        for k in range(rep.shape[1]):
            acc = np.float32(np.float64(acc) + np.float64(rep[b, k].item()) * np.float64(E[n + 1, k].item()))
        assert float(emu[b, n]) == float(acc)


@pytest.mark.parametrize("name", ["H150", "H157"])
def test_a_dropped_last_k_step_is_rejected(name):
    _rejects(name, "drop_last_kstep")


def test_a_row_taken_from_the_other_chunk_is_rejected():
    _rejects("H150", "row_xor_64")


def test_a_shifted_last_partial_tile_is_rejected():
    _rejects("H150", "shift_last_tile")                     # N = 650: the last tile holds items 641 .. 650


def test_an_operand_rounded_to_bf16_is_rejected():
    _rejects("H150", "bf16_operand")


def test_one_small_element_off_by_64_ulp_is_rejected_and_the_max_norm_accepts_it():
    rep, E, N, (s, t), emu = _built("H150")
    dev = _rejects("H150", "small_element_64ulp")
    changed = torch.nonzero(dev != emu)
    assert changed.shape[0] == 1
    b, n = changed[0].tolist()
    assert abs(float(emu[b, n])) < 1e-3 * float(emu.abs().max())        # a small-magnitude logit
    # the criterion that held Engine.logits before this module: one max-norm over the tensor, bound 1e-4
    assert _nerr(dev, s) < 1e-4 / 10                                    # ... with a factor of ten to spare


# ------------------------------------------------------------------------------------------- row log-sum-exp
def _rows(ncols, ld, dominant, seed=9):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(6, ld, generator=g) * 0.6
    x[1, 0] = dominant
    x[2, ncols - 1] = dominant
    x[:, ncols:] = float("nan")                              # beyond ncols: never read
    return x


@pytest.mark.parametrize("ncols", [1, 255, 256, 257, 650, 4097])
def test_row_lse_emulation_passes_its_own_check(ncols):
    x = _rows(ncols, ncols + 5, 80.0)
    emu = G.row_lse_emulate(x, ncols)
    err, base, bound = G.check_row_lse(emu.clone(), x, ncols, emu=emu)
    assert err == base and base < 2.0 ** -20 and bool(torch.isfinite(emu).all())
    assert abs(float(emu[1]) - 80.0) < 1e-3 and abs(float(emu[2]) - 80.0) < 1e-3 or ncols == 1


def test_row_lse_maximum_one_column_short_is_rejected():
    ncols = 650
    x = _rows(ncols, ncols + 5, 100.0)
    ok = G.row_lse_emulate(x, ncols)
    G.check_row_lse(ok, x, ncols)
    with pytest.raises(X.ParityError) as ei:
        G.check_row_lse(G.row_lse_emulate(x, ncols, fault="max_short"), x, ncols)
    assert re.search(r"rows 2 \(", str(ei.value)), str(ei.value)          # the row whose dominant entry is the last column


@pytest.mark.parametrize("ncols", [256, 650])
def test_row_lse_dropped_last_partial_is_rejected(ncols):
    x = _rows(ncols, ncols + 5, 0.5)
    with pytest.raises(X.ParityError):
        G.check_row_lse(G.row_lse_emulate(x, ncols, fault="drop_partial"), x, ncols)


def test_stable_ranks_counts_ties_by_item_id():
    lg = np.array([[1.0, 2.0, 1.0, 2.0, 0.5]], dtype=np.float32)
    assert [int(G.stable_ranks(lg, [t])[0]) for t in (1, 2, 3, 4, 5)] == [2, 0, 3, 1, 4]
