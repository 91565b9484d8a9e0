#!/usr/bin/env python3
"""Top-K recommendation, fused (Engine.recommend) against the composition a caller had to write before it existed.

    python tools/bench_topk.py [--check] [--reps 3] [--warmup 1] [--rows 1024] [--k 20] [--datasets YOOCHOOSE,DIGINETICA]
                               [--train_steps 200] [--cand | --wide | --lists | --stats] [--out profiles/topk.txt]

(A) Engine.recommend(seq, k, N): ader_topk_items -- k_topk_tile (logit tiles + per-row selection in LDS) and k_topk_merge;
(B) Engine.logits(seq, N) followed by torch.topk(.., k): dense [n, N] logits in HBM, then torch's selection.  (B) is the yardstick.
(C) Engine.recommend(seq, k, N, dtype="x3"): ader_topk_items_x3 -- k_lx3t (x3 logits on the bf16 matrix cores + a per-row superset of
    the top-k in LDS) and k_topk3_finish (merge, exact recheck of the kept pairs, selection).  Its yardstick is (A) of the same run.
Shapes: --rows sessions at the catalog sizes of the two datasets (N = 25,750 and 43,105) and at N = 10^6, each on an Engine of that
catalog size at its initial weights with synthetic sessions (random lengths, uniform ids), as tools/bench_eval.py builds its synthetic
shape; --datasets adds the first --rows rows of the last test period of the shipped datasets on an Engine after --train_steps steps
on the first period (tools/bench_eval.py's model: the x3 band scales with the largest table-row norm, and an initial Gaussian table
flatters it).  One process; after a warm-up (A), (B) and (C) alternate inside every repetition; device events around the whole call (session
forward, launches, the copy back), medians.  The kernels of (A) are timed by torch.profiler over one more call; k_topk_tile is set
against its two bounds: 2 n N H over the f32 MFMA peak (157.3 TFLOP/s, v_mfma_f32_16x16x4_f32) and N H 4 bytes per 64-row chunk over
the HBM peak (8 TB/s) -- the larger one binds; k_lx3t against 3 x 2 n N H over the bf16 MFMA peak (2.5 PFLOP/s) and against k_topk_tile
of the same run.  --check asserts that (C) equals (A) bytewise, that the items of (A) and (B) agree on every row whose k-th and (k+1)-th
scores of (B) differ (torch.topk does not promise an order among ties) and that the scores agree bitwise there.

--cand measures the candidate-list form instead (default --out profiles/topk_cand.txt), per catalog size and for evenly spread lists
of M = N/100, N/10 and N ids:
(D) Engine.recommend_among(seq, k, list, N): ader_topk_items_cand -- k_topk_cand (the list's table rows gathered into the logit
    tiles) and k_topk_merge; the list is a sorted int32 host array, its copy to the device is inside the timed call;
(A) Engine.recommend over the whole catalog, and (B') Engine.logits + masked_fill(-inf) outside the list + torch.topk, the composition
    a caller writes without (D): the two yardsticks of the same run, alternating with (D) inside every repetition.
k_topk_cand is set against the larger of 2 n M H over the f32 MFMA peak and M H 4 bytes per 64-row chunk over the HBM peak; --check
asserts that the items and score bits of (D) equal those of (B') on every row whose k-th and (k+1)-th scores of (B') differ.

--wide measures the wide form instead (default --out profiles/topk_wide.txt), per catalog size and dataset:
(W) Engine.recommend_wide(seq, k, N) at k = 64, 256 and 1024: ader_topk_items_wide -- k_topk_wide_tile (logit tiles, every key that
    beats the row's threshold appended to the row's list in global memory) and k_topk_wide_select (the list cut to its best k after
    every slab), with its scratch bytes, slab count and last_topk_stats;
(B) Engine.logits + torch.topk(k), the only route to such a k without (W), and (A) Engine.recommend at k = 64 against (W) at k = 64:
    the yardsticks, alternating with (W) inside every repetition.
The two wide kernels are timed by torch.profiler over one more call, beside k_topk_tile at the same N in the same run; --check asserts
that the items and score bits of (W) equal those of (B) on every row whose k-th and (k+1)-th scores of (B) differ, and that (W) at
k = 64 equals (A) bytewise.

--lists measures the forms whose list differs from row to row instead (default --out profiles/topk_lists.txt), per catalog size and
for C = 101 (a target and 100 sampled negatives) and C = 1,024 distinct random ids per row:
(P) Engine.score_items(seq, ids, N): ader_score_items -- k_rowlist<STORE>, 64 positions of one row's list per workgroup, its table
    rows gathered;
(Q) Engine.recommend_per_row(seq, k, ids, N): ader_topk_items_rows -- k_rowlist<KEYS> and k_topk_merge;
(A) Engine.logits + torch.gather, the composition a caller writes without (P), over as many rows as keep its [n, N] logits under
    0.8 GB; every leg is reported per row.  The three alternate inside every repetition.
k_rowlist<STORE> is timed by torch.profiler over one more call and its gathered bytes per second set against the HBM probe of
profiles/; --check asserts that the scores of (P) equal those of (A) bitwise.

--stats measures top-K with the row's normaliser instead (default --out profiles/topk_stats.txt), per catalog size:
(S) Engine.recommend_stats(seq, k, N): ader_topk_items_stats -- k_topk_tile_stats (k_topk_tile's walk with the per-lane log-sum-exp and
    entropy states), k_topk_merge and k_stats_merge;
(R) Engine.row_stats(seq, N): ader_row_stats -- k_row_stats (the same walk without the row buffer) and k_stats_merge;
(A) Engine.recommend(dtype="f32") and (L) Engine.row_losses on the same rows, the only matrix-free route to a log-sum-exp without (S):
    the yardsticks.  The legs alternate inside every repetition, (A) runs twice per repetition and the spread of its runs is what
    (A) + (L) - (S), the time the fusion saves, is set against.  The kernels are timed by torch.profiler over one more call each.
--check asserts that items / scores of (S) equal (A) bytewise, that lse / entropy of (S) equal (R) bitwise, and that row_losses agrees
with lse - score_items to 1e-4."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ader_amd._lib import call  # noqa: E402
from ader_amd.engine import Engine  # noqa: E402
from ader_amd.engine.infer import TOPK_X3_BAND  # noqa: E402

PEAK_F32_MFMA, PEAK_BF16_MFMA, PEAK_HBM = 157.3e12, 2.5e15, 8.0e12
T, H = 50, 150
_out = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if _out:
        _out[0].write(line + "\n")
        _out[0].flush()


def ev_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, r


def composed(eng, seq, N, k):
    """What a caller writes without Engine.recommend: dense logits, torch.topk, the copy back.  k + 1 columns: --check needs the next score."""
    lg = eng.logits(seq, N)
    v, i = torch.topk(lg, min(k + 1, N), dim=1)
    return (i + 1).to(torch.int32).cpu().numpy(), v.cpu().numpy()


def composed_cand(eng, seq, N, k, cand_d):
    """(B'): dense logits, every column outside the list to -inf, torch.topk, the copy back.  k + 1 columns, as composed()."""
    lg = eng.logits(seq, N)
    out = torch.ones(N, dtype=torch.bool, device=lg.device)
    out[cand_d.long() - 1] = False
    lg.masked_fill_(out, float("-inf"))
    v, i = torch.topk(lg, min(k + 1, N), dim=1)
    return (i + 1).to(torch.int32).cpu().numpy(), v.cpu().numpy()


def measure_cand(name, eng, seq, N, args):
    n, k = seq.shape[0], args.k
    seq_d = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    med = statistics.median
    rows = min(n, eng.MAX_ROWS)
    Bp = (rows + 63) // 64 * 64
    nchunk = sum((min(n, s + eng.MAX_ROWS) - s + 63) // 64 for s in range(0, n, eng.MAX_ROWS))
    say("== %s: %d rows, k = %d, H = %d; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, k, H, args.reps, args.warmup))
    ok = True
    for M in sorted({max(N // 100, k + 1), max(N // 10, k + 1), N}):
        cand = (np.arange(M, dtype=np.int64) * N // M + 1).astype(np.int32)          # evenly spread, ascending, distinct
        cand_d = torch.from_numpy(cand).to(eng.device)
        tA, tB, tD, b, d = [], [], [], None, None
        for it in range(args.warmup + args.reps):
            ta, _ = ev_time(lambda: eng.recommend(seq_d, k, N))
            tb, b = ev_time(lambda: composed_cand(eng, seq_d, N, k, cand_d))
            td, d = ev_time(lambda: eng.recommend_among(seq_d, k, cand, N))
            if it >= args.warmup:
                tA.append(ta)
                tB.append(tb)
                tD.append(td)
        ranges = call("ader_topk_ranges", M, Bp)
        say("  M = %d (N / %.0f), %d tiles over %d ranges" % (M, N / M, (M + 63) // 64, ranges))
        say("    (D) recommend_among          %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (%d ranges x %d rows x k keys of 8 B)" %
            (med(tD) * 1e3, min(tD) * 1e3, max(tD) * 1e3, n / med(tD), ranges * Bp * k * 8, ranges, Bp))
        say("    (A) recommend, whole catalog %9.2f ms [%.2f .. %.2f]  %9.0f rows/s" % (med(tA) * 1e3, min(tA) * 1e3, max(tA) * 1e3, n / med(tA)))
        say("    (B') logits + mask + topk    %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (the [n, N] float32 logits)" %
            (med(tB) * 1e3, min(tB) * 1e3, max(tB) * 1e3, n / med(tB), n * ((N + 3) // 4 * 4) * 4))
        say("    (D) / (A) whole call %.3f; (D) / (B') whole call %.3f  (< 1: the candidate walk is faster)" % (med(tD) / med(tA), med(tD) / med(tB)))
        kt = kernel_times(lambda: eng.recommend_among(seq_d, k, cand, N))
        tile = sum(t for nm, t in kt.items() if "k_topk_cand" in nm)
        merge = sum(t for nm, t in kt.items() if "k_topk_merge" in nm)
        b_mfma, b_hbm = 2.0 * n * M * H / PEAK_F32_MFMA, float(nchunk) * M * H * 4 / PEAK_HBM
        bound, which = max((b_mfma, "MFMA"), (b_hbm, "HBM"))
        if tile:
            say("    k_topk_cand %.3f ms, k_topk_merge %.3f ms (torch.profiler, one call); bounds: 2nMH over the f32 MFMA peak %.3f ms, M H 4 B x "
                "%d chunks over the HBM peak %.3f ms -> %s binds; k_topk_cand = %.1f x its bound" %
                (tile * 1e3, merge * 1e3, b_mfma * 1e3, nchunk, b_hbm * 1e3, which, tile / bound))
        else:
            say("    torch.profiler reported no k_topk_cand rows (kernels seen: %d): kernel time NOT measured; bounds: MFMA %.3f ms, HBM %.3f ms"
                % (len(kt), b_mfma * 1e3, b_hbm * 1e3))
        if M == N:
            kta = kernel_times(lambda: eng.recommend(seq_d, k, N))
            ta_k = sum(t for nm, t in kta.items() if "k_topk_tile" in nm)
            if ta_k and tile:
                say("    at M = N: k_topk_cand %.3f ms against k_topk_tile %.3f ms of the same run = %.2f x (what the gather costs)" %
                    (tile * 1e3, ta_k * 1e3, tile / ta_k))
        if args.check:
            ib, vb = b
            decided = vb[:, k - 1] != vb[:, k] if vb.shape[1] > k else np.ones(n, dtype=bool)
            same_items = np.array_equal(d[0][decided], ib[decided, :k])
            same_bits = np.array_equal(np.ascontiguousarray(d[1][decided]).view(np.int32), np.ascontiguousarray(vb[decided, :k]).view(np.int32))
            inside = bool(np.isin(d[0], cand).all())
            ok &= bool(same_items and same_bits and inside)
            say("    check: %d of %d rows have distinct k-th and (k+1)-th scores in (B'); on those, items equal: %s, scores bitwise equal: %s; "
                "every item of (D) is in the list: %s" % (int(decided.sum()), n, same_items, same_bits, inside))
        del cand_d
    del eng
    torch.cuda.empty_cache()
    return ok


def measure_wide(name, eng, seq, N, args):
    n = seq.shape[0]
    seq_d = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    med = statistics.median
    rows = min(n, eng.MAX_ROWS)
    Bp = (rows + 63) // 64 * 64
    cap = call("ader_topk_wide_cap")
    say("== %s: %d rows, H = %d, cap = %d; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, H, cap, args.reps, args.warmup))
    kta = kernel_times(lambda: eng.recommend(seq_d, 64, N, dtype="f32"))
    tile_a = sum(t for nm, t in kta.items() if "k_topk_tile" in nm)
    ok = True
    for k in (64, 256, 1024):
        tW, tB, tA, w, b, a = [], [], [], None, None, None
        for it in range(args.warmup + args.reps):
            tw, w = ev_time(lambda: eng.recommend_wide(seq_d, k, N))
            st = dict(eng.last_topk_stats)
            tb, b = ev_time(lambda: composed(eng, seq_d, N, k))
            if k == 64:
                ta, a = ev_time(lambda: eng.recommend(seq_d, k, N, dtype="f32"))
            if it >= args.warmup:
                tW.append(tw)
                tB.append(tb)
                if k == 64:
                    tA.append(ta)
        say("  k = %d: %d slabs" % (k, st["slabs"]))
        say("    (W) recommend_wide          %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (%d rows x cap keys of 8 B + 16 B per row)" %
            (med(tW) * 1e3, min(tW) * 1e3, max(tW) * 1e3, n / med(tW), Bp * cap * 8 + Bp * 16, Bp))
        say("    (B) logits + torch.topk     %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (the [n, N] float32 logits)" %
            (med(tB) * 1e3, min(tB) * 1e3, max(tB) * 1e3, n / med(tB), n * ((N + 3) // 4 * 4) * 4))
        say("    (W) / (B) whole call %.3f  (< 1: the wide path is faster)" % (med(tW) / med(tB)))
        if k == 64:
            say("    (A) recommend, k = 64       %9.2f ms [%.2f .. %.2f]  %9.0f rows/s; (W) / (A) whole call %.3f" %
                (med(tA) * 1e3, min(tA) * 1e3, max(tA) * 1e3, n / med(tA), med(tW) / med(tA)))
        say("    (W) last_topk_stats %r%s" % (st, "  ** max_list above cap / 2 **" if st["max_list"] > cap // 2 else ""))
        if st["overflowed_rows"]:
            say("    ** %d rows overflowed at the default cap and were recomputed **" % st["overflowed_rows"])
        kt = kernel_times(lambda: eng.recommend_wide(seq_d, k, N))
        tile = sum(t for nm, t in kt.items() if "k_topk_wide_tile" in nm)
        sel = sum(t for nm, t in kt.items() if "k_topk_wide_select" in nm)
        if tile and tile_a:
            say("    k_topk_wide_tile %.3f ms, k_topk_wide_select %.3f ms over %d slabs (torch.profiler, one call); k_topk_tile (k = 64) at the "
                "same N in the same run %.3f ms: wide tile / k_topk_tile = %.2f x, wide tile + select / k_topk_tile = %.2f x" %
                (tile * 1e3, sel * 1e3, st["slabs"], tile_a * 1e3, tile / tile_a, (tile + sel) / tile_a))
        else:
            say("    torch.profiler reported no k_topk_wide_tile / k_topk_tile rows (kernels seen: %d, %d): kernel time NOT measured" %
                (len(kt), len(kta)))
        if args.check:
            ib, vb = b
            kk = min(k, vb.shape[1])
            decided = vb[:, k - 1] != vb[:, k] if vb.shape[1] > k else np.ones(n, dtype=bool)
            same_items = np.array_equal(w[0][decided, :kk], ib[decided, :kk])
            same_bits = np.array_equal(np.ascontiguousarray(w[1][decided, :kk]).view(np.int32),
                                       np.ascontiguousarray(vb[decided, :kk]).view(np.int32))
            ok &= bool(same_items and same_bits)
            say("    check: %d of %d rows have distinct k-th and (k+1)-th scores in (B); on those, items equal: %s, scores bitwise equal: %s" %
                (int(decided.sum()), n, same_items, same_bits))
            if k == 64:
                same_a = (np.array_equal(w[0], a[0]) and
                          np.array_equal(np.ascontiguousarray(w[1]).view(np.int32), np.ascontiguousarray(a[1]).view(np.int32)))
                ok &= bool(same_a)
                say("    check: (W) at k = 64 equals (A) bytewise: %s" % same_a)
    del eng
    torch.cuda.empty_cache()
    return ok


def composed_gather(eng, seq, N, ids_d):
    """(A) of --lists: what a caller writes without Engine.score_items -- dense [n, N] logits, torch.gather at the listed ids, the copy
    back.  (ids in [1, N] only: the composition has no rule for the others.)"""
    lg = eng.logits(seq, N)
    return torch.gather(lg, 1, ids_d.long() - 1).cpu().numpy()


def measure_lists(name, eng, seq, N, args):
    n, k = seq.shape[0], args.k
    med = statistics.median
    ldo = (N + 3) // 4 * 4
    nA = max(1, min(n, 200_000_000 // ldo))              # rows whose dense logits stay under 0.8 GB
    seq_d = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    say("== %s: %d rows ((A): %d rows, 0.8 GB of logits at most, reported per row), k = %d, H = %d; %d repetitions after %d warm-up, "
        "medians [min .. max]" % (name, n, nA, k, H, args.reps, args.warmup))
    ok = True
    rs = np.random.default_rng(1)
    for C in (101, 1024):
        # every row its own list: C distinct random ids, ascending (recommend_per_row's form; score_items takes them as they are)
        ids = np.stack([np.sort(rs.choice(N, size=C, replace=False)) + 1 for _ in range(n)]).astype(np.int32)
        ids_d = torch.from_numpy(ids).to(eng.device)
        tP, tQ, tA, p, a = [], [], [], None, None
        for it in range(args.warmup + args.reps):
            tp, p = ev_time(lambda: eng.score_items(seq_d, ids_d, N))
            tq, _ = ev_time(lambda: eng.recommend_per_row(seq_d, k, ids, N))
            ta, a = ev_time(lambda: composed_gather(eng, seq_d[:nA], N, ids_d[:nA]))
            if it >= args.warmup:
                tP.append(tp)
                tQ.append(tq)
                tA.append(ta)
        us = lambda ts, rows: (med(ts) / rows * 1e6, min(ts) / rows * 1e6, max(ts) / rows * 1e6)
        say("  C = %d ids per row" % C)
        say("    (P) score_items              %9.2f ms  %9.3f us/row [%.3f .. %.3f]" % ((med(tP) * 1e3,) + us(tP, n)))
        say("    (Q) recommend_per_row        %9.2f ms  %9.3f us/row [%.3f .. %.3f]   (the host's check of the lists' form is inside the call)"
            % ((med(tQ) * 1e3,) + us(tQ, n)))
        say("    (A) logits + torch.gather    %9.2f ms  %9.3f us/row [%.3f .. %.3f]   over %d rows; scratch %d B (the [n, N] float32 logits)"
            % ((med(tA) * 1e3,) + us(tA, nA) + (nA, nA * ldo * 4)))
        say("    per row: (P) / (A) = %.4f, (Q) / (A) = %.4f  (< 1: the gathered walk is faster)" %
            (med(tP) / n / (med(tA) / nA), med(tQ) / n / (med(tA) / nA)))
        kt = kernel_times(lambda: eng.score_items(seq_d, ids_d, N))
        row = sum(t for nm, t in kt.items() if "k_rowlist" in nm)
        if row:
            say("    k_rowlist<STORE> %.3f ms (torch.profiler, one call): %d x %d table rows of %d B gathered = %.2f TB/s "
                "(streaming reads of the HBM probe, profiles/bw_probe2_r2z.txt: 5.7 - 6.2 TB/s)" %
                (row * 1e3, n, C, H * 4, n * C * H * 4.0 / row / 1e12))
        else:
            say("    torch.profiler reported no k_rowlist rows (kernels seen: %d): kernel time NOT measured" % len(kt))
        if args.check:
            same = np.array_equal(np.ascontiguousarray(p[:nA]).view(np.int32), np.ascontiguousarray(a).view(np.int32))
            ok &= bool(same)
            say("    check: the scores of (P) equal those of (A) bitwise on its %d rows: %s" % (nA, same))
        del ids_d
    del eng
    torch.cuda.empty_cache()
    return ok


def measure_stats(name, eng, seq, N, args):
    n, k = seq.shape[0], args.k
    seq_d = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    pos_d = torch.from_numpy(np.random.RandomState(1).randint(1, N + 1, size=n).astype(np.int32)).to(eng.device)
    med = statistics.median
    rows = min(n, eng.MAX_ROWS)
    Bp = (rows + 63) // 64 * 64
    ranges = call("ader_topk_ranges", N, Bp)
    tA, tA2, tL, tS, tR, a, s, r = [], [], [], [], [], None, None, None
    for it in range(args.warmup + args.reps):
        ta, a = ev_time(lambda: eng.recommend(seq_d, k, N, dtype="f32"))
        tl, _ = ev_time(lambda: eng.row_losses(seq_d, pos_d, N).cpu())
        ts, s = ev_time(lambda: eng.recommend_stats(seq_d, k, N))
        tr, r = ev_time(lambda: eng.row_stats(seq_d, N))
        ta2, _ = ev_time(lambda: eng.recommend(seq_d, k, N, dtype="f32"))
        if it >= args.warmup:
            tA.append(ta)
            tA2.append(ta2)
            tL.append(tl)
            tS.append(ts)
            tR.append(tr)
    allA = tA + tA2
    spread = max(allA) - min(allA)
    say("== %s: %d rows, k = %d, H = %d; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, k, H, args.reps, args.warmup))
    say("  (A) recommend                %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   twice per repetition: spread (max - min) of its %d runs %.3f ms"
        % (med(allA) * 1e3, min(allA) * 1e3, max(allA) * 1e3, n / med(allA), len(allA), spread * 1e3))
    say("  (L) row_losses               %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   the parent's matrix-free route to a log-sum-exp" %
        (med(tL) * 1e3, min(tL) * 1e3, max(tL) * 1e3, n / med(tL)))
    say("  (S) recommend_stats          %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (%d ranges x %d rows x (k keys of 8 B + 16 B))" %
        (med(tS) * 1e3, min(tS) * 1e3, max(tS) * 1e3, n / med(tS), ranges * Bp * (k * 8 + 16), ranges, Bp))
    say("  (R) row_stats                %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B" %
        (med(tR) * 1e3, min(tR) * 1e3, max(tR) * 1e3, n / med(tR), ranges * Bp * 16))
    gain = med(allA) + med(tL) - med(tS)
    say("  (S) / (A) whole call %.3f; (A) + (L) - (S) = %.3f ms = %.1f x the spread of (A): the fusion %s; (R) / (A) %.3f" %
        (med(tS) / med(allA), gain * 1e3, gain / spread if spread > 0 else float("inf"),
         "pays" if gain > spread else "does NOT pay beyond the spread", med(tR) / med(allA)))
    kts = kernel_times(lambda: eng.recommend_stats(seq_d, k, N))
    kta = kernel_times(lambda: eng.recommend(seq_d, k, N, dtype="f32"))
    ktr = kernel_times(lambda: eng.row_stats(seq_d, N))
    pick = lambda kt, key: sum(t for nm, t in kt.items() if key in nm and (key != "k_topk_tile" or "k_topk_tile_stats" not in nm))
    if pick(kts, "k_topk_tile_stats") and pick(kta, "k_topk_tile"):
        say("  kernels (torch.profiler, one call each): k_topk_tile_stats %.3f ms + k_topk_merge %.3f ms + k_stats_merge %.3f ms; k_topk_tile of "
            "(A) %.3f ms: tile_stats / tile = %.3f; k_row_stats %.3f ms + k_stats_merge %.3f ms" %
            (pick(kts, "k_topk_tile_stats") * 1e3, pick(kts, "k_topk_merge") * 1e3, pick(kts, "k_stats_merge") * 1e3,
             pick(kta, "k_topk_tile") * 1e3, pick(kts, "k_topk_tile_stats") / pick(kta, "k_topk_tile"), pick(ktr, "k_row_stats") * 1e3,
             pick(ktr, "k_stats_merge") * 1e3))
    else:
        say("  torch.profiler reported no k_topk_tile_stats / k_topk_tile rows (kernels seen: %d, %d): kernel time NOT measured" %
            (len(kts), len(kta)))
    ok = True
    if args.check:
        same = (np.array_equal(a[0], s[0]) and np.array_equal(np.ascontiguousarray(a[1]).view(np.int32), np.ascontiguousarray(s[1]).view(np.int32)))
        same_r = (np.array_equal(s[2].view(np.int32), r[0].view(np.int32)) and np.array_equal(s[3].view(np.int32), r[1].view(np.int32)))
        loss = eng.row_losses(seq_d, pos_d, N).cpu().numpy()
        mine = s[2] - eng.score_items(seq_d, pos_d[:, None].contiguous(), N)[:, 0]
        err = float(np.abs(loss - mine).max())
        ok = bool(same and same_r and err < 1e-4)
        say("  check: items / scores of (S) equal (A) bytewise: %s; lse / entropy of (S) equal (R) bitwise: %s; max |row_losses - (lse - "
            "score)| = %.3g; entropy in [%.4f, %.4f] nats of log N = %.4f" % (same, same_r, err, s[3].min(), s[3].max(), np.log(N)))
    del eng
    torch.cuda.empty_cache()
    return ok


def kernel_times(fn):
    """Device time per kernel name over one call of fn (torch.profiler); {} if the profiler reports no kernels."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        t = getattr(e, "device_time_total", None)
        if t is None:
            t = getattr(e, "cuda_time_total", 0.0)
        if t:
            out[e.key] = out.get(e.key, 0.0) + t * 1e-6
    return out


def synthetic(N, args):
    n = args.rows
    eng = Engine(N, maxlen=T, hidden_units=H, num_blocks=2, num_heads=1, seed=0)
    rs = np.random.RandomState(0)
    seq = np.zeros((n, T), dtype=np.int32)
    for b in range(n):
        ln = int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, N + 1, size=ln)
    return (measure_cand if args.cand else measure_wide if args.wide else measure_lists if args.lists else measure_stats if args.stats
            else measure)("N = %d" % N, eng, seq, N, args)


def dataset(name, args):
    """The first --rows rows the Evaluator ranks in the last test period, on tools/bench_eval.py's briefly trained model."""
    import random

    from bench_eval import evaluator_rows
    from ader_amd.data import DataLoader, Sampler
    from ader_amd.main import ITEM_NUM
    dl = DataLoader(name)
    periods = dl.num_periods() - 1
    eng = Engine(ITEM_NUM[name], maxlen=T, hidden_units=H, num_blocks=2, num_heads=1, seed=0)
    random.seed(0)
    np.random.seed(0)
    for period in range(1, periods + 1):
        train_sess, _ = dl.train_loader(period - 1)
        test_sess, _ = dl.evaluate_loader(period)
        N = dl.max_item()
        if period == 1 and args.train_steps:
            smp = Sampler(train_sess, T, 256)
            for _ in range(min(args.train_steps, smp.batch_num())):
                seq, pos = smp.next_batch()
                if len(pos) == 256:
                    eng.train_step(seq, pos, N, 5e-4, rate=0.3)
            torch.cuda.synchronize()
    seq, _ = evaluator_rows(test_sess, N, 1024)
    return (measure_wide if args.wide else measure)("%s, test period %d, N = %d, %d training steps" % (name, periods, N, args.train_steps), eng,
                                                    seq[:args.rows], N, args)


def measure(name, eng, seq, N, args):
    n, k = seq.shape[0], args.k
    seq_d = torch.from_numpy(np.ascontiguousarray(seq)).to(eng.device)
    tA, tB, tC, a, b, c = [], [], [], None, None, None
    for it in range(args.warmup + args.reps):
        ta, a = ev_time(lambda: eng.recommend(seq_d, k, N))
        tb, b = ev_time(lambda: composed(eng, seq_d, N, k))
        tc, c = ev_time(lambda: eng.recommend(seq_d, k, N, dtype="x3"))
        if it >= args.warmup:
            tA.append(ta)
            tB.append(tb)
            tC.append(tc)
    st3 = dict(eng.last_topk_stats or {})
    tf = statistics.median(ev_time(lambda: eng.encode(seq_d))[0] for _ in range(args.reps))
    med = statistics.median
    rows = min(n, eng.MAX_ROWS)
    Bp = (rows + 63) // 64 * 64
    ranges = call("ader_topk_ranges", N, Bp)
    Bp3 = (rows + 127) // 128 * 128
    ranges3 = call("ader_topk_x3_ranges", N, Bp3)
    say("== %s: %d rows, k = %d, H = %d; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, k, H, args.reps, args.warmup))
    say("  (A) Engine.recommend       %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (%d ranges x %d rows x k keys of 8 B)" %
        (med(tA) * 1e3, min(tA) * 1e3, max(tA) * 1e3, n / med(tA), ranges * Bp * k * 8, ranges, Bp))
    say("  (B) logits + torch.topk    %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (the [n, N] float32 logits)" %
        (med(tB) * 1e3, min(tB) * 1e3, max(tB) * 1e3, n / med(tB), n * ((N + 3) // 4 * 4) * 4))
    say("  (C) recommend dtype=x3     %9.2f ms [%.2f .. %.2f]  %9.0f rows/s   scratch %12d B (%d ranges x %d rows x (k + band) keys of 8 B)" %
        (med(tC) * 1e3, min(tC) * 1e3, max(tC) * 1e3, n / med(tC), ranges3 * Bp3 * (k + TOPK_X3_BAND) * 8, ranges3, Bp3))
    say("  (A) / (B) whole call %.3f  (< 1: the fused path is faster); (C) / (A) whole call %.3f  (< 1: x3 is faster); session forward "
        "(encode) alone %.2f ms" % (med(tA) / med(tB), med(tC) / med(tA), tf * 1e3))
    say("  (C) last_topk_stats %r: %.2f kept pairs per row" % (st3, st3.get("kept_pairs", 0) / max(n, 1)))
    kt = kernel_times(lambda: eng.recommend(seq_d, k, N))
    tile = sum(t for name, t in kt.items() if "k_topk_tile" in name)
    merge = sum(t for name, t in kt.items() if "k_topk_merge" in name)
    nchunk = sum((min(n, s + eng.MAX_ROWS) - s + 63) // 64 for s in range(0, n, eng.MAX_ROWS))
    b_mfma, b_hbm = 2.0 * n * N * H / PEAK_F32_MFMA, float(nchunk) * N * H * 4 / PEAK_HBM
    bound, which = max((b_mfma, "MFMA"), (b_hbm, "HBM"))
    if tile:
        say("  k_topk_tile %.3f ms, k_topk_merge %.3f ms (torch.profiler, one call); bounds: 2nNH over the f32 MFMA peak %.3f ms, N H 4 B x %d "
            "chunks over the HBM peak %.3f ms -> %s binds; k_topk_tile = %.1f x its bound" %
            (tile * 1e3, merge * 1e3, b_mfma * 1e3, nchunk, b_hbm * 1e3, which, tile / bound))
    else:
        say("  torch.profiler reported no k_topk_tile rows (kernels seen: %d): kernel time NOT measured; bounds: MFMA %.3f ms, HBM %.3f ms "
            "-> %s binds" % (len(kt), b_mfma * 1e3, b_hbm * 1e3, which))
    kt3 = kernel_times(lambda: eng.recommend(seq_d, k, N, dtype="x3"))
    filt = sum(t for nm, t in kt3.items() if "k_lx3t" in nm)
    fin = sum(t for nm, t in kt3.items() if "k_topk3_finish" in nm)
    b3 = 3.0 * 2.0 * n * N * H / PEAK_BF16_MFMA
    if filt:
        say("  k_lx3t %.3f ms, k_topk3_finish %.3f ms (torch.profiler, one call); bound: 3 x 2nNH over the bf16 MFMA peak %.3f ms; k_lx3t = "
            "%.1f x its bound%s" % (filt * 1e3, fin * 1e3, b3 * 1e3, filt / b3, ", %.2f x k_topk_tile" % (filt / tile) if tile else ""))
    else:
        say("  torch.profiler reported no k_lx3t rows (kernels seen: %d): kernel time NOT measured; bound %.3f ms" % (len(kt3), b3 * 1e3))
    ok = True
    if args.check:
        same_c = (np.array_equal(a[0], c[0]) and
                  np.array_equal(np.ascontiguousarray(a[1]).view(np.int32), np.ascontiguousarray(c[1]).view(np.int32)))
        say("  check: (C) equals (A) bytewise (items and score bits): %s" % same_c)
        ok = bool(same_c)
        ib, vb = b
        decided = vb[:, k - 1] != vb[:, k] if vb.shape[1] > k else np.ones(n, dtype=bool)
        kk = min(k, vb.shape[1])
        same_items = np.array_equal(a[0][decided, :kk], ib[decided, :kk])
        same_bits = np.array_equal(np.ascontiguousarray(a[1][decided, :kk]).view(np.int32), np.ascontiguousarray(vb[decided, :kk]).view(np.int32))
        ok &= bool(same_items and same_bits)
        say("  check: %d of %d rows have distinct k-th and (k+1)-th scores; on those, items equal: %s, scores bitwise equal: %s" %
            (int(decided.sum()), n, same_items, same_bits))
    del eng
    torch.cuda.empty_cache()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="assert that (A) and (B) return the same items wherever (B)'s order is decided")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--catalogs", default="25750,43105,1000000")
    ap.add_argument("--datasets", default="", help="e.g. YOOCHOOSE,DIGINETICA: also the last test period of these, on a briefly trained model")
    ap.add_argument("--train_steps", type=int, default=200)
    ap.add_argument("--cand", action="store_true", help="measure the candidate-list form: legs (D), (A) and (B') at M = N/100, N/10 and N")
    ap.add_argument("--wide", action="store_true", help="measure the wide form: legs (W) at k = 64, 256, 1024, (B) and (A)")
    ap.add_argument("--lists", action="store_true", help="measure the per-row list form: legs (P) score_items and (Q) recommend_per_row at "
                                                       "C = 101 and 1,024 ids per row against (A) logits + torch.gather")
    ap.add_argument("--stats", action="store_true", help="measure top-K with the row's log-sum-exp and entropy: legs (S) recommend_stats and "
                                                       "(R) row_stats against (A) recommend and (L) row_losses")
    ap.add_argument("--out", default=None, help="default: profiles/topk.txt, profiles/topk_cand.txt with --cand, profiles/topk_wide.txt with "
                                                "--wide, profiles/topk_lists.txt with --lists, profiles/topk_stats.txt with --stats")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                "topk_cand.txt" if args.cand else "topk_wide.txt" if args.wide else "topk_lists.txt" if args.lists
                                else "topk_stats.txt" if args.stats else "topk.txt")
    if args.cand + args.wide + args.lists + args.stats > 1:
        raise SystemExit("--cand, --wide, --lists and --stats are four measurements: run them one at a time")
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_topk.py measures on the GPU: no device found")
    _out.append(open(args.out, "w"))
    if args.cand:
        if args.datasets:
            raise SystemExit("--cand measures the synthetic catalogs only")
        say("# tools/bench_topk.py --cand%s: (D) Engine.recommend_among (k_topk_cand + k_topk_merge) against (A) Engine.recommend over "
            "the whole catalog and (B') Engine.logits + mask + torch.topk, same process, alternating; %s" %
            (" --check" if args.check else "", torch.cuda.get_device_name(0)))
        ok = True
        for N in [int(x) for x in args.catalogs.split(",") if x]:
            ok &= synthetic(N, args)
        say("# (D) equal to (B') wherever the yardstick's order is decided: %s" % (ok if args.check else "not checked"))
        if args.check and not ok:
            raise SystemExit("top-K mismatch between (D) and (B')")
        return
    if args.stats:
        if args.datasets:
            raise SystemExit("--stats measures the synthetic catalogs only")
        say("# tools/bench_topk.py --stats%s: (S) Engine.recommend_stats (k_topk_tile_stats + k_topk_merge + k_stats_merge) and (R) "
            "Engine.row_stats (k_row_stats + k_stats_merge) against (A) Engine.recommend and (L) Engine.row_losses, same process, "
            "alternating; %s" % (" --check" if args.check else "", torch.cuda.get_device_name(0)))
        ok = True
        for N in [int(x) for x in args.catalogs.split(",") if x]:
            ok &= synthetic(N, args)
        say("# items / scores of (S) equal to (A) bytewise, lse / entropy of (S) equal to (R) bitwise: %s" % (ok if args.check else "not checked"))
        if args.check and not ok:
            raise SystemExit("mismatch between (S) and its yardsticks")
        return
    if args.lists:
        if args.datasets:
            raise SystemExit("--lists measures the synthetic catalogs only")
        say("# tools/bench_topk.py --lists%s: (P) Engine.score_items and (Q) Engine.recommend_per_row (k_rowlist, + k_topk_merge) over random "
            "lists of C ids per row against (A) Engine.logits + torch.gather, same process, alternating; %s" %
            (" --check" if args.check else "", torch.cuda.get_device_name(0)))
        ok = True
        for N in [int(x) for x in args.catalogs.split(",") if x]:
            ok &= synthetic(N, args)
        say("# (P) equal to (A) bitwise: %s" % (ok if args.check else "not checked"))
        if args.check and not ok:
            raise SystemExit("score mismatch between (P) and (A)")
        return
    if args.wide:
        say("# tools/bench_topk.py --wide%s: (W) Engine.recommend_wide (k_topk_wide_tile + k_topk_wide_select) at k = 64, 256, 1024 against "
            "(B) Engine.logits + torch.topk and (A) Engine.recommend at k = 64, same process, alternating; %s" %
            (" --check" if args.check else "", torch.cuda.get_device_name(0)))
        ok = True
        for N in [int(x) for x in args.catalogs.split(",") if x]:
            ok &= synthetic(N, args)
        for name in [d for d in args.datasets.split(",") if d]:
            ok &= dataset(name, args)
        say("# (W) equal to (B) wherever the yardstick's order is decided, (W) at k = 64 equal to (A) bytewise: %s" %
            (ok if args.check else "not checked"))
        if args.check and not ok:
            raise SystemExit("top-K mismatch between (W) and its yardsticks")
        return
    say("# tools/bench_topk.py%s: (A) Engine.recommend (k_topk_tile + k_topk_merge) against (B) Engine.logits + torch.topk and (C) "
        "Engine.recommend(dtype=\"x3\") (k_lx3t + k_topk3_finish), same process, alternating; %s" %
        (" --check" if args.check else "", torch.cuda.get_device_name(0)))
    ok = True
    for N in [int(x) for x in args.catalogs.split(",") if x]:
        ok &= synthetic(N, args)
    for name in [d for d in args.datasets.split(",") if d]:
        ok &= dataset(name, args)
    say("# (C) equal to (A) bytewise, (A) equal to (B) wherever the yardstick's order is decided: %s" % (ok if args.check else "not checked"))
    if args.check and not ok:
        raise SystemExit("top-K mismatch between the three legs")


if __name__ == "__main__":
    main()
