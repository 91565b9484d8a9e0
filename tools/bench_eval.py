#!/usr/bin/env python3
"""Evaluation ranking, "x3" against the exact-f32 kernel (Engine.rank_targets dtype= / --rank_dtype): times, candidate shares, the bound.

    python tools/bench_eval.py [--check] [--reps 5] [--warmup 2] [--train_steps 200] [--out profiles/eval_x3.txt]
    python tools/bench_eval.py --among [...]      the candidate-list rank instead (measure_among below), to profiles/rank_cand.txt

Shapes: (a) the last test period of data/YOOCHOOSE.npz and data/DIGINETICA.npz -- the rows the product's DataLoader / Evaluator hand to
model.rank_targets; (b) 4,096 synthetic rows at N = 10^6.  Per shape and dtype, device events around (1) the whole rank_targets call
(session forward, rank launches, the copy back) and (2) the rank launches alone on precomputed representations; the two dtypes alternate
inside every repetition, medians over the repetitions after a warm-up.  The rank launches are set against 2 B N H over the peak of the
matrix arithmetic they use: 157.3 TFLOP/s (v_mfma_f32_16x16x4_f32) for "f32", three bf16 MFMAs per product at 2.5 PFLOP/s for "x3".
--check also asserts ranks(x3) == ranks(f32) on every test period of both datasets.  The model is an Engine at its initial weights after
--train_steps steps on the first period: enough for the table norms and target logits to leave the init symmetry, not a trained model."""
import argparse
import os
import random
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from ader_amd._lib import ptr  # noqa: E402
from ader_amd.data import DataLoader, Evaluator, Sampler  # noqa: E402
from ader_amd.engine import Engine  # noqa: E402
from ader_amd.engine import infer_launch as L  # noqa: E402
from ader_amd.engine.infer import RANK_X3_CAND_PER_ROW  # noqa: E402
from ader_amd.main import ITEM_NUM  # noqa: E402

PEAK_F32_MFMA, PEAK_BF16_MFMA = 157.3e12, 2.5e15
T, H = 50, 150
_out = []


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if _out:
        _out[0].write(line + "\n")
        _out[0].flush()


class _Capture:
    """Stands where the model does in an Evaluator: keeps the rows the Evaluator would rank."""

    def rank_targets(self, seq, pos, max_item):
        self.seq, self.pos = np.ascontiguousarray(seq, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.int32)
        return np.zeros(len(pos), dtype=np.int32)


def evaluator_rows(sessions, max_item, batch):
    cap = _Capture()
    ev = Evaluator(sessions, False, T, batch, max_item, "test", cap, None)
    ev.evaluate(0)
    return cap.seq, cap.pos


def ev_time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3, r


def rank_launches(eng, rep, pos, N, dtype):
    """The rank launches of Engine.rank_targets alone, on precomputed representations (no forward, no copy back)."""
    ws, st, emb = L.fresh(rep.device), torch.cuda.current_stream().cuda_stream, ptr(eng.param("emb"))
    n = rep.shape[0]
    if dtype == "x3":
        emax = L.rank_emax(ws, st, emb, eng.item_num, eng.H, N)
    for s in range(0, n, eng.MAX_ROWS):
        e = min(n, s + eng.MAX_ROWS)
        if dtype == "x3":
            L.rank_targets_x3(ws, st, rep[s:e], emb, eng.item_num, eng.H, N, pos[s:e], emax, RANK_X3_CAND_PER_ROW * L.pad_rows(e - s, 128))
        else:
            L.rank_targets(ws, st, rep[s:e], emb, eng.H, N, pos[s:e])


def measure(name, eng, seq, pos, N, reps, warmup):
    n = len(pos)
    seq_d = torch.from_numpy(seq).to(eng.device)
    pos_d = torch.from_numpy(pos).to(eng.device)
    rep = eng.encode(seq_d)
    whole, launches, fwd, ranks, stats = {"f32": [], "x3": []}, {"f32": [], "x3": []}, [], {}, None
    for it in range(warmup + reps):
        for dt in ("f32", "x3"):                                   # alternating inside every repetition
            t, r = ev_time(lambda: eng.rank_targets(seq_d, pos_d, N, dtype=dt))
            tl, _ = ev_time(lambda: rank_launches(eng, rep, pos_d, N, dt))
            if it >= warmup:
                whole[dt].append(t)
                launches[dt].append(tl)
            ranks[dt] = r
            if dt == "x3":
                stats = dict(eng.last_rank_stats)
        tf, _ = ev_time(lambda: eng.encode(seq_d))
        if it >= warmup:
            fwd.append(tf)
    equal = bool(np.array_equal(ranks["f32"], ranks["x3"]))
    flop = 2.0 * n * N * eng.H
    med = statistics.median
    say("== %s: %d rows, N = %d, H = %d; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, N, eng.H, reps, warmup))
    for dt, ideal in (("f32", flop / PEAK_F32_MFMA), ("x3", 3.0 * flop / PEAK_BF16_MFMA)):
        w, l = whole[dt], launches[dt]
        say("  %-3s  rank_targets %9.2f ms [%.2f .. %.2f]  %9.0f rows/s | rank launches %9.2f ms [%.2f .. %.2f] = %5.1f x the %.3f ms of "
            "2BNH%s over the MFMA peak" % (dt, med(w) * 1e3, min(w) * 1e3, max(w) * 1e3, n / med(w), med(l) * 1e3, min(l) * 1e3, max(l) * 1e3,
                                          med(l) / ideal, ideal * 1e3, " x 3" if dt == "x3" else ""))
    say("  session forward (encode) %.2f ms = %.0f %% of the f32 call, %.0f %% of the x3 call" %
        (med(fwd) * 1e3, 100 * med(fwd) / med(whole["f32"]), 100 * med(fwd) / med(whole["x3"])))
    say("  x3 / f32: whole call %.3f, rank launches %.3f  (< 1: x3 is faster)" %
        (med(whole["x3"]) / med(whole["f32"]), med(launches["x3"]) / med(launches["f32"])))
    say("  last_rank_stats %r; candidate share %.3e; %.1f candidates per row (default cap 64 per padded row); ranks equal: %s" %
        (stats, stats["candidates"] / max(stats["pairs"], 1), stats["candidates"] / max(n, 1), equal))
    return equal


def among_launches(eng, rep, pos, seq, N, cand, exclude):
    """The rank launches of Engine.rank_targets_among alone, on precomputed representations (no forward, no copy back)."""
    ws, st, emb = L.fresh(rep.device), torch.cuda.current_stream().cuda_stream, ptr(eng.param("emb"))
    n = rep.shape[0]
    for s in range(0, n, eng.MAX_ROWS):
        e = min(n, s + eng.MAX_ROWS)
        L.rank_targets_cand(ws, st, rep[s:e], emb, eng.H, N, pos[s:e], cand, seq[s:e] if exclude else None, eng.status)


def torch_among(eng, seq, pos, N, cand, exclude):
    """What a user composes without the kernel: dense Engine.logits, the list, the seen ids and the target's column masked out, the
    count of (lg > tl) | (lg == tl and id < t) -- in row groups whose logits stay near 1 GB."""
    dev, n = eng.device, seq.shape[0]
    listed = torch.zeros(N + 1, dtype=torch.bool, device=dev)
    listed[cand.long()] = True
    ids = torch.arange(1, N + 1, device=dev)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    group = max(1, 256_000_000 // N)
    for s in range(0, n, group):
        e = min(n, s + group)
        lg = eng.logits(seq[s:e], N)
        t = pos[s:e].long()
        tl = lg.gather(1, (t - 1)[:, None])
        ahead = ((lg > tl) | ((lg == tl) & (ids[None, :] < t[:, None]))) & listed[None, 1:]
        ahead.scatter_(1, (t - 1)[:, None], False)
        if exclude:
            sid = seq[s:e].long()
            sid = torch.where(sid <= N, sid, torch.zeros_like(sid))                  # column 0 = "no id" (and ids above N)
            ahead = torch.cat([torch.zeros((e - s, 1), dtype=torch.bool, device=dev), ahead], 1)
            ahead.scatter_(1, sid, False)
        out[s:e] = ahead.sum(1)
    return out.cpu().numpy()


def measure_among(name, eng, seq, pos, N, reps, warmup):
    """--among: rank_targets_among over a random tenth of the ids and over all ids, against rank_targets (f32) and against the torch
    composition for the tenth, alternating inside every repetition.  The work of k_rank_cand follows the list: the tenth should cost
    well under the whole-catalog rank launches; what is printed is what was measured."""
    n = len(pos)
    seq_d, pos_d = torch.from_numpy(seq).to(eng.device), torch.from_numpy(pos).to(eng.device)
    rep = eng.encode(seq_d)
    rs = np.random.RandomState(0)
    tenth = np.sort(rs.choice(N, size=max(N // 10, 1), replace=False)).astype(np.int32) + 1
    lists = {"tenth": torch.from_numpy(tenth).to(eng.device), "all": torch.arange(1, N + 1, dtype=torch.int32, device=eng.device)}
    calls = {"rank_targets f32": lambda: eng.rank_targets(seq_d, pos_d, N, dtype="f32"),
             "among all ids": lambda: eng.rank_targets_among(seq_d, pos_d, N, lists["all"]),
             "among N/10": lambda: eng.rank_targets_among(seq_d, pos_d, N, lists["tenth"]),
             "among N/10, seen excluded": lambda: eng.rank_targets_among(seq_d, pos_d, N, lists["tenth"], exclude_seen=True),
             "torch logits+mask+count N/10": lambda: torch_among(eng, seq_d, pos_d, N, lists["tenth"], False)}
    launches = {"rank_targets f32": lambda: rank_launches(eng, rep, pos_d, N, "f32"),
                "among all ids": lambda: among_launches(eng, rep, pos_d, seq_d, N, lists["all"], False),
                "among N/10": lambda: among_launches(eng, rep, pos_d, seq_d, N, lists["tenth"], False),
                "among N/10, seen excluded": lambda: among_launches(eng, rep, pos_d, seq_d, N, lists["tenth"], True)}
    tw, tl, res = {k: [] for k in calls}, {k: [] for k in launches}, {}
    for it in range(warmup + reps):
        for k in calls:                                                # alternating inside every repetition
            t, res[k] = ev_time(calls[k])
            if it >= warmup:
                tw[k].append(t)
            if k in launches:
                t, _ = ev_time(launches[k])
                if it >= warmup:
                    tl[k].append(t)
    eng.check_status()
    med = statistics.median
    say("== %s: %d rows, N = %d, list of %d ids; %d repetitions after %d warm-up, medians [min .. max]" % (name, n, N, len(tenth), reps, warmup))
    for k in calls:
        w = tw[k]
        line = "  %-30s whole call %9.2f ms [%.2f .. %.2f]" % (k, med(w) * 1e3, min(w) * 1e3, max(w) * 1e3)
        if k in launches:
            l = tl[k]
            line += " | rank launches %9.3f ms [%.3f .. %.3f]" % (med(l) * 1e3, min(l) * 1e3, max(l) * 1e3)
        say(line)
    base = med(tl["rank_targets f32"])
    say("  rank launches over rank_targets f32's: among all ids %.3f, among N/10 %.3f, among N/10 seen excluded %.3f; whole call, torch "
        "composition over among N/10: %.1f" % (med(tl["among all ids"]) / base, med(tl["among N/10"]) / base,
                                              med(tl["among N/10, seen excluded"]) / base,
                                              med(tw["torch logits+mask+count N/10"]) / med(tw["among N/10"])))
    ok = bool(np.array_equal(res["among all ids"], res["rank_targets f32"]))
    ok &= bool(np.array_equal(res["among N/10"], res["torch logits+mask+count N/10"]))
    ok &= bool(np.array_equal(res["among N/10, seen excluded"], torch_among(eng, seq_d, pos_d, N, lists["tenth"], True)))
    say("  among all ids == rank_targets, among N/10 == the torch composition (with and without seen ids): %s" % ok)
    return ok


def dataset(name, args):
    """Measures the last test period; returns (ok, check) where check() compares the two dtypes on every earlier test period."""
    dl = DataLoader(name)
    periods = dl.num_periods() - 1
    eng = Engine(ITEM_NUM[name], maxlen=T, hidden_units=H, num_blocks=2, num_heads=1, seed=0)
    random.seed(0)
    np.random.seed(0)
    rows = []
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
        if period == periods or args.check:
            rows.append((period, N) + evaluator_rows(test_sess, N, args.eval_batch))
    period, N, seq, pos = rows.pop()
    ok = (measure_among if args.among else measure)("%s, test period %d" % (name, period), eng, seq, pos, N, args.reps, args.warmup)

    def check():
        good = True
        for period, N, seq, pos in rows:
            a = eng.rank_targets(seq, pos, N, dtype="f32")
            b = eng.rank_targets(seq, pos, N, dtype="x3")
            eq = bool(np.array_equal(a, b))
            say("  check %s period %2d: %6d rows, N = %5d, ranks equal: %s, %r" % (name, period, len(pos), N, eq, eng.last_rank_stats))
            good &= eq
        return good
    return ok, check


def synthetic(args):
    N, B = 1_000_000, args.synthetic_rows
    eng = Engine(N, maxlen=T, hidden_units=H, num_blocks=2, num_heads=1, seed=0)
    rs = np.random.RandomState(0)
    seq = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        ln = int(rs.randint(1, T + 1))
        seq[b, T - ln:] = rs.randint(1, N + 1, size=ln)
    pos = rs.randint(1, N + 1, size=B).astype(np.int32)
    return (measure_among if args.among else measure)("synthetic", eng, seq, pos, N, max(args.reps // 2, 2), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="assert rank equality of the two dtypes on every test period of both datasets")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--train_steps", type=int, default=200)
    ap.add_argument("--eval_batch", type=int, default=1024)
    ap.add_argument("--synthetic_rows", type=int, default=4096)
    ap.add_argument("--datasets", default="YOOCHOOSE,DIGINETICA")
    ap.add_argument("--among", action="store_true", help="measure Engine.rank_targets_among (k_rank_cand) over a list of N/10 and of all "
                    "ids against rank_targets f32 and against Engine.logits + mask + count in torch; writes profiles/rank_cand.txt")
    ap.add_argument("--out", default=None, help="profiles/eval_x3.txt, with --among profiles/rank_cand.txt")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_eval.py measures on the GPU: no device found")
    if args.among and args.check:
        raise SystemExit("--check compares the two rank dtypes: not with --among")
    _out.append(open(args.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                              "rank_cand.txt" if args.among else "eval_x3.txt"), "w"))
    if args.among:
        say("# tools/bench_eval.py --among: Engine.rank_targets_among (k_rank_cand, gathered tiles) over a random tenth of the ids and over "
            "all ids, against Engine.rank_targets f32 (k_logits_tile<RANK>) and dense logits + mask + count in torch, same process, "
            "alternating; %s" % torch.cuda.get_device_name(0))
    else:
        say("# tools/bench_eval.py%s: Engine.rank_targets, dtype x3 (k_lx3k filter + exact recheck) against f32 (k_logits_tile<RANK>), "
            "same process, alternating; %s" % (" --check" if args.check else "", torch.cuda.get_device_name(0)))
    ok, checks = True, []
    for name in [d for d in args.datasets.split(",") if d]:
        good, check = dataset(name, args)
        ok &= good
        checks.append(check)
    if args.synthetic_rows:
        ok &= synthetic(args)
    for check in checks:                                           # (the measurements first: the checks are the long part)
        ok &= check()
    say("# ranks equal everywhere: %s" % ok)
    if args.among and not ok:
        raise SystemExit("rank mismatch between rank_targets_among and its references")
    if args.check and not ok:
        raise SystemExit("rank mismatch between x3 and f32")


if __name__ == "__main__":
    main()
