"""Self-checks of the catalog-sharded half of oracle/x3_step_ref.py, the reference behind tests/test_gpu_x3_shard_rowwise.py (CPU only).
emulate(shards=...) -- per-shard {M, L, O} partials merged in rank order -- must stay inside the bound the UNSHARDED emulation sets
on every SHARD_CASES entry (the merge order does not consume the factor 8), the inputs must hold the conditions the cases are about,
the padded-layout helper must round-trip, and each of ten planted faults of the sharded scheme must be rejected by check() or by the
bitwise row checks.  The faults confined to one item, one shard's readout or the label row (a shard clipped one item short of N or
of Np, a readout partial under its own lse, the label row in bf16) are also put through the theta measure of tests/test_gpu_dp.py,
which lets them pass: from zero Adam state the update is lr_t m / (sqrt(v) + eps) = +-lr for every element whose gradient exceeds
eps, whatever its size, so a small relative fault of the gradient leaves theta where it was."""
import functools

import numpy as np
import pytest
import torch

from oracle import x3_step_ref as X

CASE = {c["name"]: c for c in X.SHARD_CASES}
K = X.adam_consts(5e-4, np.float32(0.9), np.float32(0.999))


@functools.lru_cache(maxsize=None)
def _built(name):
    """(case, batch, inputs, reference, unsharded emulation, sharded emulation) of a case: computed once, shared, never modified."""
    case = CASE[name]
    batch = X.make_shard_batch(case)
    inp = X.shard_inputs_of(case, batch, *X.synth_upstream(X.flat_case(case), batch))
    return case, batch, inp, X.reference(inp), X.emulate(inp), X.emulate(inp, shards=X.shards_of(case))


def _as_dev(emu, **over):
    d = {k: emu[k].clone() if torch.is_tensor(emu[k]) else emu[k] for k in ("lse", "rowloss", "loss", "drep", "g")}
    d.update(over)
    return d


def _faulty(name, fault, frow=None):
    case, _, inp, _, _, _ = _built(name)
    return X.emulate(inp, shards=X.shards_of(case), fault=fault, frow=frow)


def _rejects(name, bad, quantity):
    """check() under the bound of the sharded emulation -- the GPU test's bound -- rejects `bad`, naming `quantity`."""
    _, _, inp, ref, _, emu = _built(name)
    with pytest.raises(X.ParityError) as ei:
        X.check(_as_dev(bad), inp, ref=ref, emu=emu)
    assert quantity in str(ei.value), str(ei.value)


def _theta_after(name, g):
    """theta after ONE Adam step from zero state with table gradient g (the whole table: rows 0 and > N included)."""
    _, _, inp, _, _, _ = _built(name)
    z = torch.zeros_like(inp["E0"])
    return torch.from_numpy(X.adam_emulate(inp["E0"], z, z, g, inp["N"], K)[0])


def _passes_dp_bound(name, bad):
    """The fault survives the measure of test_two_ranks_match_single_process (99.5 % within 5e-6, max < 2.5e-3)."""
    _, _, _, _, _, emu = _built(name)
    return X.dp_theta_bound_passes(_theta_after(name, bad["g"]), _theta_after(name, emu["g"]))


# ------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", X.SHARD_CASE_IDS)
def test_sharded_emulation_stays_inside_the_unsharded_bound(name):
    case, batch, inp, ref, emu0, emu = _built(name)
    assert X.dense_only_condition(inp) is None, X.dense_only_condition(inp)
    res = X.check(_as_dev(emu), inp, ref=ref, emu=emu0)                 # bound: the UNSHARDED emulation's
    assert set(res) == set(X.QUANTITIES)
    for q, (err, base, bound) in res.items():
        assert base < 2.0 ** -13, (q, base)
    lim = torch.full((inp["B"],), inp["N"])
    if inp["tl"] is not None:
        lim[inp["n_train"]:] = inp["Np"]
    X.check_empty_parts(emu["parts"], X.shards_of(case), lim)
    # the real rows carry step_weights of the GLOBAL counts, label-0 rows and rows without a teacher row weight 0
    W, B, n_ex = case["W"], case["B"], case["n_ex"]
    real_t = batch["pos"] > 0
    n_t = int(real_t.sum())
    n_e = int((batch["trow"] >= 0).sum()) if n_ex else 0
    sw = X.step_weights(n_t, n_e, case["lam"])
    assert n_t == W * B - sum(case["pads"].values())
    assert torch.equal(inp["w"][:W * B][torch.as_tensor(real_t)], sw[:n_t]) and not bool(inp["w"][:W * B][torch.as_tensor(~real_t)].any())
    if n_ex:
        real_e = torch.as_tensor(batch["trow"] >= 0)
        assert torch.equal(inp["w"][W * B:][real_e], sw[n_t:]) and not bool(inp["w"][W * B:][~real_e].any())


@pytest.mark.parametrize("name", ["W2_N650", "W3_kd_Np645_ex24", "W3_B70_label0"])
def test_one_shard_over_all_items_is_the_unsharded_emulation(name):
    """shards = [(0, N)]: one partial, merged with the factor exp2(0) = 1 -- nothing is regrouped, every output is bit-identical."""
    _, _, inp, _, emu0, _ = _built(name)
    one = X.emulate(inp, shards=[(0, inp["N"])])
    for q in ("lse", "rowloss", "loss", "drep", "g", "c"):
        assert torch.equal(one[q], emu0[q]), q
    assert len(one["parts"]) == 1


def test_case_conditions():
    sh = {n: X.shard_table_rows(X.shards_of(c), c["N"]) for n, c in CASE.items()}
    assert sh["W2_N650"] == [(1, 384), (385, 650)] and (650 - 384) % 64 != 0           # clipped, its last tile partial
    assert sh["W3_N257"] == [(1, 256), (257, 257), (1, 0)]                             # one item, then an empty shard
    assert sh["W3_N256"] == [(1, 256), (1, 0), (1, 0)]                                 # N on the boundary
    assert sh["W3_N320"] == [(1, 256), (257, 320), (1, 0)]                             # a single 64-row tile: its partner is beyond the range
    assert sh["W8_N650"][5] == (641, 650) and sh["W8_N650"][6:] == [(1, 0), (1, 0)]
    assert sh["W2_N2"] == [(1, 2), (1, 0)]
    for n, c in CASE.items():
        assert c["S"] % 128 == 0 and c["W"] * c["S"] >= c["item_num"] > c["W"] * (c["S"] - 128) and c["N"] <= c["item_num"]
        lay = X.padded_layout(c["W"], c["B"], c["n_ex"])
        assert lay["Bg"] <= 2048 + 1024
    assert X.padded_layout(2, 128)["Bg"] == 256 and not bool(X.padding_rows(X.padded_layout(2, 128)).any())
    assert int(X.padding_rows(X.padded_layout(2, 129)).sum()) == 2 * 127
    assert X.padded_layout(8, 129)["Bg"] == 2048 and X.padded_layout(2, 700)["Bg"] == 1536
    # label-0 rows: at the end of the MIDDLE block and of the last one
    _, batch, inp, _, _, _ = _built("W3_B70_label0")
    assert list(np.nonzero(batch["pos"] == 0)[0]) == [139, 209] and not batch["seq"][[139, 209]].any()
    assert float(inp["w"][139]) == 0.0 and float(inp["w"][138]) == float(np.float32(1.0 / 208))
    # distilled: a row without a teacher row inside every rank's exemplar block (a real row, or the block's own padding rows)
    for n, c in CASE.items():
        if c["mode"] != "kd":
            continue
        _, batch, inp, _, _, _ = _built(n)
        lay = X.padded_layout(c["W"], c["B"], c["n_ex"])
        tr = X.to_padded(torch.cat([torch.zeros(c["W"] * c["B"], dtype=torch.int32), torch.as_tensor(batch["trow"])]), lay, fill=-1)
        blocks = tr[c["W"] * lay["Bp"]:].view(c["W"], lay["Bk"])
        assert bool((blocks < 0).any(-1).all()) and bool((blocks >= 0).any(-1).all()), n
        if c["n_ex"] >= 2:
            assert bool((torch.as_tensor(batch["trow"]).view(c["W"], c["n_ex"]) < 0).any(-1).all()), n
        assert 1 <= c["Np"] <= c["N"]
    assert CASE["W3_kd_Np645_ex24"]["Np"] % 4 and CASE["W3_kd_Np257_ex24"]["Np"] - CASE["W3_kd_Np257_ex24"]["S"] == 1
    # sparse lists: hot id 400 sits in the first tile of shard 1; the packed form hands a rank only the ids it owns
    c = CASE["W2_lists_hot_packed"]
    _, batch, _, _, _, _ = _built("W2_lists_hot_packed")
    assert c["S"] == 384 and (400 - 1) // c["S"] == 1 and (400 - 1 - c["S"]) // X.TI == 0 and int((batch["seq"] == 400).sum()) == 250
    own = X.owner_of(batch["seq"].reshape(-1), c)
    assert set(np.unique(own)) == {-1, 0, 1} and (own == 0).sum() >= 600 and (own == 1).sum() >= 270


@pytest.mark.parametrize("W,B,n_ex", [(2, 128, 0), (3, 70, 0), (3, 24, 129), (8, 129, 1), (1, 1, 1)])
def test_padded_layout_round_trips(W, B, n_ex):
    lay = X.padded_layout(W, B, n_ex)
    n = W * (B + n_ex)
    x = torch.arange(1, n + 1, dtype=torch.float32)
    p = X.to_padded(x, lay, fill=-7.0)
    assert p.shape == (lay["Bg"],) and lay["Bg"] % 128 == 0 and torch.equal(X.from_padded(p, lay), x)
    pad = X.padding_rows(lay)
    assert int(pad.sum()) == lay["Bg"] - n and bool((p[pad] == -7.0).all()) and len(set(lay["rows"].tolist())) == n
    # rank d's train rows sit in block d, its exemplar rows in block d behind the W train blocks
    for d in range(W):
        assert torch.equal(p[d * lay["Bp"]:d * lay["Bp"] + B], x[d * B:(d + 1) * B])
        k0 = W * lay["Bp"] + d * lay["Bk"]
        assert torch.equal(p[k0:k0 + n_ex], x[W * B + d * n_ex:W * B + (d + 1) * n_ex])
    x2 = torch.randn(n, 3)
    assert torch.equal(X.from_padded(X.to_padded(x2, lay), lay), x2)


# ------------------------------------------------------------------------------------------- planted faults: the forward
def test_rejects_a_shard_clipped_one_item_short_of_N():
    bad = _faulty("W2_N650", "clip_N")
    _rejects("W2_N650", bad, "lse")
    assert _passes_dp_bound("W2_N650", bad)


def test_rejects_a_shard_clipped_one_item_short_of_Np():
    bad = _faulty("W3_kd_Np645_ex24", "clip_Np")
    _rejects("W3_kd_Np645_ex24", bad, "lse")
    assert _passes_dp_bound("W3_kd_Np645_ex24", bad)


def test_rejects_partials_merged_without_the_rescale():
    _rejects("W2_N650", _faulty("W2_N650", "no_rescale"), "lse")


def test_rejects_an_empty_shards_max_taken_as_zero():
    """Merged with {0, 0, zeros} the result is the same up to rounding while the logits stay near zero -- check() cannot see it --
    but the partial itself is not what an empty shard has to send: the bitwise check of the partials rejects it."""
    case, _, inp, ref, _, emu = _built("W3_N257")
    bad = _faulty("W3_N257", "empty_M0")
    X.check(_as_dev(bad), inp, ref=ref, emu=emu)
    with pytest.raises(X.ParityError) as ei:
        X.check_empty_parts(bad["parts"], X.shards_of(case), torch.full((inp["B"],), inp["N"]))
    assert "empty shard 2" in str(ei.value)


def test_rejects_the_exemplar_softmax_of_one_shard_run_over_N():
    case, _, inp, _, _, _ = _built("W3_kd_Np257_ex24")
    bad = _faulty("W3_kd_Np257_ex24", "ex_over_N", frow=1)              # shard 1: items 257..512, one of them below Np
    _rejects("W3_kd_Np257_ex24", bad, "lse")


def test_rejects_a_readout_partial_normalised_by_its_shards_own_lse():
    bad = _faulty("W3_kd_Np648_ex24", "readout_own_lse", frow=2)
    _rejects("W3_kd_Np648_ex24", bad, "drep")
    assert _passes_dp_bound("W3_kd_Np648_ex24", bad)


def test_rejects_the_label_row_rounded_to_bf16():
    bad = _faulty("W2_N650", "label_bf16")
    _rejects("W2_N650", bad, "rowloss")
    assert _passes_dp_bound("W2_N650", bad)


def test_rejects_a_middle_block_padding_row_with_weight():
    _, _, inp, _, _, _ = _built("W3_B70_label0")
    bad = _faulty("W3_B70_label0", "pad_weight", frow=139)             # the label-0 row at the end of rank 1's block
    _rejects("W3_B70_label0", bad, "g_dense")
    with pytest.raises(X.ParityError) as ei:
        X.check(_as_dev(bad), inp, ref=_built("W3_B70_label0")[3], emu=_built("W3_B70_label0")[5])
    assert "rowloss" in str(ei.value) and "139" in str(ei.value)
    assert not bool(torch.isneginf(bad["off"][139])) and bool(torch.isneginf(_built("W3_B70_label0")[5]["off"][139]))


# ------------------------------------------------------------------------------------------- planted faults: the range update
def _range_run(name, fault=None, frank=None, preloaded=False):
    case, _, inp, _, _, emu = _built(name)
    th0 = inp["E0"]
    m0, v0 = torch.zeros_like(th0), torch.zeros_like(th0)
    if preloaded:
        g = torch.Generator().manual_seed(5)
        m0 = torch.randn(th0.shape, generator=g) * 1e-3
        v0 = torch.rand(th0.shape, generator=g) * 1e-6
    snaps = X.range_update_emulate(th0, m0, v0, emu["g"], inp["N"], K, X.shards_of(case), fault=fault, frank=frank)
    return case, inp, emu, (th0.numpy(), m0.numpy(), v0.numpy()), snaps


def _range_checks(case, inp, before, snaps):
    prev = before
    for r, (lo, hi) in enumerate(X.shard_table_rows(X.shards_of(case), inp["N"])):
        X.check_range_untouched(prev, snaps[r], lo, hi, r)
        prev = snaps[r]
    X.check_untouched(before, snaps[-1], inp["N"])


@pytest.mark.parametrize("name", ["W2_N650", "W3_N320", "W3_N256", "W8_N650"])
@pytest.mark.parametrize("preloaded", [False, True])
def test_range_launches_add_up_to_the_whole_update(name, preloaded):
    case, inp, emu, before, snaps = _range_run(name, preloaded=preloaded)
    _range_checks(case, inp, before, snaps)
    whole = X.adam_emulate(*before, emu["g"], inp["N"], K)
    for a, b in zip(whole, snaps[-1]):
        assert np.array_equal(a, b)
    if not preloaded:
        g_dev = X.check_adam_zero(before[0], snaps[-1][0], snaps[-1][1], snaps[-1][2], inp["N"], K)
        assert float((g_dev - emu["g"].double()).abs().max()) <= 2.0 ** -23 * float(emu["g"].abs().max())
    else:
        X.check_adam_preloaded(*before, *snaps[-1], emu["g"].double(), inp["N"], K)


def test_rejects_a_range_update_that_drops_a_shards_first_tile():
    case, inp, emu, before, snaps = _range_run("W2_N650", fault="drop_first_tile", frank=1)
    _range_checks(case, inp, before, snaps)                             # nothing was written that should not be
    g_dev = X.check_adam_zero(before[0], snaps[-1][0], snaps[-1][1], snaps[-1][2], inp["N"], K)
    assert not bool(g_dev[384:448].any()) and bool(g_dev[448:].any())
    _rejects("W2_N650", _as_dev(emu, g=g_dev), "g_dense")
    with pytest.raises(X.ParityError) as ei:
        X.check(_as_dev(emu, g=g_dev), inp, ref=_built("W2_N650")[3], emu=emu)
    assert "worst rows" in str(ei.value) and any(("%d (" % i) in str(ei.value) for i in range(385, 449))


def test_rejects_a_range_update_that_writes_the_tile_after_tile_end():
    for name, frank, row in (("W2_N650", 0, 385), ("W3_N320", 1, None)):
        case, inp, emu, before, snaps = _range_run(name, fault="tile_after_end", frank=frank)
        if row is None:                                                 # the tile behind shard 1 of W3_N320 lies beyond N: nothing to write
            _range_checks(case, inp, before, snaps)
            continue
        with pytest.raises(X.ParityError) as ei:
            _range_checks(case, inp, before, snaps)
        assert "rank %d's launch" % frank in str(ei.value) and "wrote row %d" % row in str(ei.value)
    # preloaded state makes the second update of those rows visible to the Adam check too
    case, inp, emu, before, snaps = _range_run("W2_N650", fault="tile_after_end", frank=0, preloaded=True)
    with pytest.raises(X.ParityError):
        X.check_adam_preloaded(*before, *snaps[-1], emu["g"].double(), inp["N"], K)
