"""The launch layer of the inference family (include/ader_hip.h, ader_logits_store .. ader_topk_items_stats): one plain function per
launcher, the only place in ader_amd/ and tools/ that calls it.  Engine (infer.py), the torch operators (ops.py) and the bench tools
build no argument list of their own; tests/test_infer_launch_host.py checks every list, name by name, against the prototypes.

What the functions share:
  ws(name, shape, dtype=torch.float32)  the workspace allocator.  Engine passes Engine.buf (persistent, reused across chunks); the
           operators and the tools pass fresh(device).  The buffer names are owned here, one per meaning, distinct within every call.
  st       the raw stream handle;  emb: the DEVICE ADDRESS of the item table [item_num + 1, H] (row 0 = the padding item).
  rep      float32 [B, H], contiguous;  B is read off it and padded here (stage_rows).
  seen     int32 [B, S] or None.  None passes (NULL, seen_ld = 0): the C side ignores seen_ld when seen is NULL.
  items / scores / lse / entropy / status / diag   the caller's outputs, written in place.
A function returns only what it allocated and its caller still needs: the padded rank, the row status of x3 / wide, diag."""
import torch

from .._lib import call, ptr
from .common import LDR


def fresh(device):
    """The allocator of a caller without persistent workspace: a new uninitialised tensor per request."""
    return lambda name, shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=device)


def pad_rows(B, pad=64):
    return (B + pad - 1) // pad * pad


def stage_rows(ws, B, N, pad=64, target=None):
    """The padded rows of one launch -> (Bp, ncol, tgt): Bp = B padded to `pad` rows (64; 128 for the x3 filters), ncol int32 [Bp] = N
    for real rows and 0 for padding rows, tgt int32 [Bp] = target for real rows and 0 for padding rows (None without a target).
    Cleared and filled on every call: nothing is cached."""
    Bp = pad_rows(B, pad)
    tgt = None
    if target is not None:
        tgt = ws("inf_tgt", (Bp,), torch.int32)
        tgt.zero_()
        tgt[:B] = target
    ncol = ws("inf_ncol", (Bp,), torch.int32)
    ncol.zero_()
    ncol[:B] = N
    return Bp, ncol, tgt


def _padded(ws, rep, N, pad=64, target=None):
    B = rep.shape[0]
    return (B,) + stage_rows(ws, B, N, pad, target)


def _rank_stage(ws, rep, N, target, pad=64):
    """_padded with a target, after the two [Bp] vectors every rank launcher fills -> (B, Bp, ncol, tgt, tlogit, rank)."""
    Bp = pad_rows(rep.shape[0], pad)
    tl, rk = ws("inf_tl", (Bp,)), ws("inf_rank", (Bp,), torch.int32)
    return _padded(ws, rep, N, pad, target) + (tl, rk)


def _seen(seen):
    return ptr(seen), seen.shape[1] if seen is not None else 0


def logits_store(ws, st, rep, emb, H, N, out):
    """out [B, N] (any row stride) = rep . E[1..N]^T."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    call("ader_logits_store", ptr(rep), emb, B, Bp, H, N, ptr(ncol), ptr(out), out.stride(0), st)


def rank_targets(ws, st, rep, emb, H, N, target):
    """-> rank int32 [Bp]: the 0-based rank of target[b] among items 1..N in [:B]."""
    B, Bp, ncol, tgt, tl, rk = _rank_stage(ws, rep, N, target)
    call("ader_rank_targets", ptr(rep), emb, B, Bp, H, N, ptr(tgt), ptr(ncol), ptr(tl), ptr(rk), st)
    return rk


def rank_emax(ws, st, emb, item_num, H, N):
    """-> emax float32 [1], what the two x3 filters scale their band by: once per call of theirs, after the table is final."""
    emax = ws("inf_emax", (1,))
    call("ader_rank_emax", emb, item_num, H, N, ptr(emax), st)
    return emax


def rank_targets_x3(ws, st, rep, emb, item_num, H, N, target, emax, cap, diag=None):
    """rank_targets through the x3 filter, rows padded to 128; cap: entries of the candidate list -> (rank int32 [Bp], diag int32 [2]):
    the ranks are valid iff diag[0] <= cap."""
    B, Bp, ncol, tgt, tl, rk = _rank_stage(ws, rep, N, target, 128)
    rep_hi, rep_lo = ws("inf_rep_hi", (Bp * LDR,), torch.bfloat16), ws("inf_rep_lo", (Bp * LDR,), torch.bfloat16)
    delta, cand = ws("inf_delta", (Bp,)), ws("inf_x3_cand", (3 * max(cap, 1),), torch.int32)
    if diag is None:
        diag = ws("inf_diag", (2,), torch.int32)
    call("ader_rank_targets_x3", ptr(rep), emb, item_num, B, Bp, H, N, ptr(tgt), ptr(ncol), ptr(rep_hi), ptr(rep_lo), ptr(tl), ptr(delta),
         ptr(emax), ptr(cand), cap, ptr(diag), ptr(rk), st)
    return rk, diag


def _part(ws, n, Bp, k):
    """The 64-bit keys of scratch of the top-K walks over n columns: ader_topk_ranges(n, Bp) * Bp * k."""
    return ws("inf_part", (call("ader_topk_ranges", n, Bp) * Bp * k,), torch.int64)


def _spart(ws, N, Bp):
    """The floats of scratch of the row statistics: ader_row_stats_floats(N, Bp)."""
    return ws("inf_spart", (call("ader_row_stats_floats", N, Bp),))


def _list(t):
    """(pointer, length) of a shared candidate list int32 [M], or (pointer, columns) of per-row lists int32 [B, C]; None or an empty
    list: (NULL, 0)."""
    n = 0 if t is None else int(t.shape[-1])
    return (ptr(t) if n else None), n


def rank_targets_cand(ws, st, rep, emb, H, N, target, cand, seen, status):
    """rank_targets over the ascending ids cand int32 [M] (None: M = 0) minus the row's seen ids -> rank int32 [Bp]."""
    B, Bp, ncol, tgt, tl, rk = _rank_stage(ws, rep, N, target)
    cand_p, M = _list(cand)
    call("ader_rank_targets_cand", ptr(rep), emb, B, Bp, H, N, ptr(tgt), ptr(ncol), cand_p, M, *_seen(seen), ptr(tl), ptr(rk),
         ptr(status), st)
    return rk


def rank_targets_rows(ws, st, rep, emb, H, N, target, ids, seen, status):
    """rank_targets_cand with row b's own list ids[b] (int32 [B, C] contiguous, ascending then 0 padding; None: C = 0) -> rank [Bp]."""
    B, Bp, ncol, tgt, tl, rk = _rank_stage(ws, rep, N, target)
    ids_p, C = _list(ids)
    call("ader_rank_targets_rows", ptr(rep), emb, B, Bp, H, N, ptr(tgt), ptr(ncol), ids_p, C, C, *_seen(seen), ptr(tl), ptr(rk),
         ptr(status), st)
    return rk


def topk_items(ws, st, rep, emb, H, N, seen, k, items, scores):
    """items int32 / scores float32 [B, k]: the k best of items 1..N per row."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    part = _part(ws, N, Bp, k)
    call("ader_topk_items", ptr(rep), emb, B, Bp, H, N, ptr(ncol), *_seen(seen), k, ptr(part), ptr(items), ptr(scores), st)


def topk_items_cand(ws, st, rep, emb, H, N, cand, seen, k, items, scores, status):
    """topk_items over the ascending ids cand int32 [M] (None: M = 0): the scratch follows M."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    cand_p, M = _list(cand)
    part = _part(ws, M, Bp, k)
    call("ader_topk_items_cand", ptr(rep), emb, B, Bp, H, N, ptr(ncol), cand_p, M, *_seen(seen), k, ptr(part), ptr(items),
         ptr(scores), ptr(status), st)


def topk_items_rows(ws, st, rep, emb, H, N, ids, seen, k, items, scores, status):
    """topk_items_cand with row b's own list ids[b] (as rank_targets_rows').  part: ader_topk_rows_ranges(C, k) * Bp * k keys."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    ids_p, C = _list(ids)
    part = ws("inf_part", (call("ader_topk_rows_ranges", C, k) * Bp * k,), torch.int64)
    call("ader_topk_items_rows", ptr(rep), emb, B, Bp, H, N, ptr(ncol), ids_p, C, C, *_seen(seen), k, ptr(part), ptr(items),
         ptr(scores), ptr(status), st)


def score_items(st, rep, emb, H, N, ids, scores):
    """scores float32 [B, C] contiguous = the logit of ids[b, c] (int32 [B, C] contiguous, any ids) for row b.  Any B: no padded stage,
    ncol = NULL (every row takes N), no workspace."""
    ids_p, C = _list(ids)
    call("ader_score_items", ptr(rep), emb, rep.shape[0], H, N, None, ids_p, C, C, ptr(scores), C, st)


def topk_items_x3(ws, st, rep, emb, item_num, H, N, seen, k, band, emax, items, scores, diag=None):
    """topk_items through the x3 filter, rows padded to 128 -> (status int32 [Bp], diag int32 [3]): a row with status != 0 outgrew
    k + band keys and takes topk_items' answer.  part3: ader_topk_x3_ranges(N, Bp) * Bp * (k + band) keys."""
    B, Bp, ncol, _ = _padded(ws, rep, N, 128)
    rep_hi, rep_lo = ws("inf_rep_hi", (Bp * LDR,), torch.bfloat16), ws("inf_rep_lo", (Bp * LDR,), torch.bfloat16)
    delta, stat = ws("inf_delta", (Bp,)), ws("inf_row_status", (Bp,), torch.int32)
    part3 = ws("inf_part3", (call("ader_topk_x3_ranges", N, Bp) * Bp * (k + band),), torch.int64)
    if diag is None:
        diag = ws("inf_diag", (3,), torch.int32)
    call("ader_topk_items_x3", ptr(rep), emb, item_num, B, Bp, H, N, ptr(ncol), *_seen(seen), k, band, ptr(rep_hi), ptr(rep_lo),
         ptr(delta), ptr(emax), ptr(part3), ptr(stat), ptr(diag), ptr(items), ptr(scores), st)
    return stat, diag


def topk_items_wide(ws, st, rep, emb, H, N, seen, k, cap, items, scores, diag=None):
    """topk_items for k up to ader_topk_wide_kmax() with cap keys of list per row -> (status int32 [Bp], diag int32 [2]): a row with
    status != 0 overflowed and is unspecified."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    lst, thr = ws("inf_list", (Bp * cap,), torch.int64), ws("inf_thr", (Bp,), torch.int64)
    cnt, stat = ws("inf_cnt", (Bp,), torch.int32), ws("inf_row_status", (Bp,), torch.int32)
    if diag is None:
        diag = ws("inf_diag", (2,), torch.int32)
    call("ader_topk_items_wide", ptr(rep), emb, B, Bp, H, N, ptr(ncol), *_seen(seen), k, cap, ptr(lst), ptr(cnt), ptr(thr),
         ptr(stat), ptr(diag), ptr(items), ptr(scores), st)
    return stat, diag


def row_stats(ws, st, rep, emb, H, N, lse, entropy):
    """lse / entropy float32 [B] of softmax over items 1..N."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    spart = _spart(ws, N, Bp)
    call("ader_row_stats", ptr(rep), emb, B, Bp, H, N, ptr(ncol), ptr(spart), ptr(lse), ptr(entropy), st)


def topk_items_stats(ws, st, rep, emb, H, N, seen, k, items, scores, lse, entropy):
    """topk_items and row_stats out of one catalog walk."""
    B, Bp, ncol, _ = _padded(ws, rep, N)
    part, spart = _part(ws, N, Bp, k), _spart(ws, N, Bp)
    call("ader_topk_items_stats", ptr(rep), emb, B, Bp, H, N, ptr(ncol), *_seen(seen), k, ptr(part), ptr(spart), ptr(items),
         ptr(scores), ptr(lse), ptr(entropy), st)
