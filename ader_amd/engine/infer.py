"""Inference paths: encode, logits, ranks (util.py:323-325), top-K items, row losses, herding selection (util.py:436-461)."""
import numpy as np
import torch

from . import infer_launch as L
from .._lib import call, ptr
from .common import TeacherRep, _check

# Half-width of the undecided band of the x3 rank filter, as a share of |rep_b| * max_n |E_n|: the SAME value as KAPPA of k_lx3k
# (csrc/logits_x3.hip, where the bound is derived).  |s_x3 - s_f32| stays below half of it; tests/test_rank_x3_host.py emulates that.
RANK_X3_KAPPA = 2.0 ** -13
RANK_X3_CAND_PER_ROW = 64      # default candidate-list entries per padded row of a chunk (Engine.rank_targets cand_cap)
RANK_DTYPES = ("f32", "x3")
TOPK_DTYPES = ("f32", "x3")
# Keys beyond k that a row of the x3 top-K filter may keep inside its band (Engine.recommend band): tests/test_topk_x3_host.py holds the
# band populations of Gaussian operands at or below half of it; at most 16 (the LDS of k_lx3t, csrc/logits_x3.hip)
TOPK_X3_BAND = 16


def _check_rank_dtype(v):
    _check(v in RANK_DTYPES, "rank_dtype must be 'f32' or 'x3' (got %r)" % (v,))
    return v


def _check_topk_dtype(v):
    _check(v in TOPK_DTYPES, "topk_dtype must be 'f32' or 'x3' (got %r)" % (v,))
    return v


def candidate_ids(candidates, N, item_num):
    """The candidate list of Engine.recommend_among in the form ader_topk_items_cand takes: a 1-D integer array or tensor of item ids ->
    sorted, unique int32 ids (numpy) that are <= N.  Ids in (N, item_num] are dropped silently, as seen ids above N are; a
    non-integer dtype, more or fewer than one dimension, or an id outside [1, item_num] raise RuntimeError."""
    if isinstance(candidates, torch.Tensor):
        a = candidates.detach().cpu().numpy()
    else:
        a = np.asarray(candidates)
        if a.size == 0 and a.ndim == 1 and not isinstance(candidates, np.ndarray):
            a = a.astype(np.int32)                           # (an empty list has no dtype of its own)
    _check(np.issubdtype(a.dtype, np.integer), "candidates must hold integers (got dtype %s)" % (a.dtype,))
    _check(a.ndim == 1, "candidates must be 1-D (got %d dimensions)" % a.ndim)
    if a.size:
        lo, hi = int(a.min()), int(a.max())
        _check(1 <= lo and hi <= item_num, "candidates must be item ids in [1, item_num = %d] (got %d .. %d)" % (item_num, lo, hi))
    if a.size > 1 and not bool(np.all(a[1:] > a[:-1])):      # (a list already in the launcher's form is not sorted again)
        a = np.unique(a)
    return np.ascontiguousarray(a[a <= N], dtype=np.int32)


def row_candidate_ids(lists, N, item_num):
    """The per-row lists of Engine.recommend_per_row / rank_targets_per_row in the form ader_topk_items_rows takes: a 2-D integer array
    or tensor (0 entries are padding), or a sequence of 1-D integer sequences -> int32 [n, C'] numpy, every row sorted, unique and
    ascending, then zero-padded; C' = the longest row (0 if every row is empty).  Ids in (N, item_num] are dropped silently; a
    non-integer dtype, a wrong rank or an id outside [0, item_num] raise RuntimeError.  A row already in form is not sorted again."""
    if isinstance(lists, torch.Tensor):
        lists = lists.detach().cpu().numpy()
    if isinstance(lists, np.ndarray):
        _check(np.issubdtype(lists.dtype, np.integer), "lists must hold integers (got dtype %s)" % (lists.dtype,))
        _check(lists.ndim == 2, "lists must be 2-D, or a sequence of 1-D sequences (got %d dimensions)" % lists.ndim)
        if lists.size:                                       # a matrix already in form, no id above N: one pass, no loop over rows
            lo, hi = int(lists.min()), int(lists.max())
            _check(0 <= lo and hi <= item_num, "lists must hold item ids in [0, item_num = %d] (got %d .. %d)" % (item_num, lo, hi))
            nxt, prv = lists[:, 1:], lists[:, :-1]
            if hi <= N and bool(np.all((nxt == 0) | ((prv > 0) & (nxt > prv)))):
                C = int(np.count_nonzero(lists, axis=1).max())
                return np.ascontiguousarray(lists[:, :C], dtype=np.int32)
        rows = list(lists)
    else:
        rows = []
        for r in lists:
            a = r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else np.asarray(r)
            if a.size == 0 and a.ndim == 1 and not isinstance(r, (np.ndarray, torch.Tensor)):
                a = a.astype(np.int32)                       # (an empty list has no dtype of its own)
            _check(np.issubdtype(a.dtype, np.integer), "lists must hold integers (got dtype %s)" % (a.dtype,))
            _check(a.ndim == 1, "every row of lists must be 1-D (got %d dimensions)" % a.ndim)
            rows.append(a)
    out = []
    for a in rows:
        if a.size:
            lo, hi = int(a.min()), int(a.max())
            _check(0 <= lo and hi <= item_num, "lists must hold item ids in [0, item_num = %d] (got %d .. %d)" % (item_num, lo, hi))
        nz = int(np.count_nonzero(a))
        head = a[:nz]
        if not (bool(np.all(head > 0)) and (nz < 2 or bool(np.all(head[1:] > head[:-1])))):      # (not: ascending ids, then the zeros)
            head = np.unique(a[a > 0])
        out.append(head[head <= N])
    C = max((len(r) for r in out), default=0)
    res = np.zeros((len(out), C), dtype=np.int32)
    for i, r in enumerate(out):
        res[i, :len(r)] = r
    return res


def log_probs(scores, lse):
    """The log-probabilities of an answer: scores float32 [n,k] (any top-K call's, or score_items') and lse float32 [n] (row_stats',
    recommend_stats') -> scores - lse[:, None], one float32 subtraction per entry; a padding score (-inf) stays -inf.  The
    distribution is the softmax over all of 1..max_item: items a call excluded keep their mass."""
    s, z = np.asarray(scores, dtype=np.float32), np.asarray(lse, dtype=np.float32)
    _check(s.ndim == 2 and z.ndim == 1 and z.shape[0] == s.shape[0],
           "log_probs: scores must be [n, k] and lse [n] (got %s and %s)" % (s.shape, z.shape))
    return s - z[:, None]


def probs(scores, lse):
    """exp(log_probs(scores, lse)) in float32: the model's probability of every returned item, 0 for padding.  They need not sum to 1
    over an answer (the items left out, excluded ones included, hold the rest)."""
    return np.exp(log_probs(scores, lse))


def rank_x3_supports(H):
    """Hidden sizes of k_lx3k (lx3f_supports of csrc/logits_x3.hip)."""
    return H % 2 == 0 and 8 <= H <= 160 and H % 8 in (0, 4, 6)


class _Packed:
    """The answer of a top-K call as ONE int32 device tensor, items [n,k] | score bits [n,k] | extras ..., so that it comes back in one
    copy.  rows(s, e) gives the device views items[s:e] (int32) / scores[s:e] (float32) for a launch to write into, extra[i] the
    i-th extra as an int32 vector; cpu() returns the same views of the host copy.  (Built from as few tensor operations as the layout
    allows: each costs the host 1 - 2 us, and the calls on short batches are host-bound.)"""

    def __init__(self, dev, n, k, extras=(), zero=False):
        self.shape, self.extras = (2, n, k), extras
        self.dev = (torch.zeros if zero else torch.empty)(2 * n * k + sum(extras), dtype=torch.int32, device=dev)
        self.both, self.extra = self._split(self.dev)
        self.scores = self.both[1].view(torch.float32)

    def _split(self, t):
        if not self.extras:
            return t.reshape(self.shape), ()
        o = 2 * self.shape[1] * self.shape[2]
        cuts = [o]
        for m in self.extras:
            cuts.append(cuts[-1] + m)
        return t[:o].reshape(self.shape), [t[a:b] for a, b in zip(cuts, cuts[1:])]

    def rows(self, s, e):
        return self.both[0, s:e], self.scores[s:e]

    def cpu(self):
        both, extra = self._split(self.dev.cpu().numpy())
        return (both[0], both[1].view(np.float32), *extra)


class _Infer:
    last_topk_stats = None     # Engine.recommend(dtype="x3"): kept_pairs, rows, overflowed_rows, fallback_chunks, max_err_over_delta of the last call
    last_rank_stats = None     # Engine.rank_targets(dtype="x3"): candidates, pairs, overflowed_chunks, max_err_over_delta of the last call

    # ---------------------------------------------------------------------------------------- what every entry point shares
    def _enter(self, seq):
        """The prelude of a public inference call, after its host checks: this call's stream, a whole table, seq on the device."""
        self._refresh_stream()
        self.sync_table()
        return self._seq_in(seq)

    def _chunks(self, seq, rep_all=None):
        """(s, e, B, rep) over chunks of MAX_ROWS rows: rep = the eval-mode forward of seq[s:e].  rep_all [n, H], if given, keeps every
        chunk's rep (rep is then its slice): what a fallback after the copy back works on."""
        n = seq.shape[0]
        for s in range(0, n, self.MAX_ROWS):
            e = min(n, s + self.MAX_ROWS)
            rep = self.forward(seq[s:e], training=False)
            if rep_all is not None:
                rep_all[s:e] = rep
                rep = rep_all[s:e]
            yield s, e, e - s, rep

    def _check_kN(self, name, max_item, k=None, kmax=None):
        """max_item (None: the whole catalog) and, if given, k against kmax, under the calling method's name -> N or (k, N)."""
        N = self.item_num if max_item is None else int(max_item)
        if k is not None:
            k = int(k)
            _check(1 <= k <= kmax, "%s: k must be in 1..%d (got %d)" % (name, kmax, k))
        _check(1 <= N <= self.item_num, "%s: max_item must be in 1..%d (got %d)" % (name, self.item_num, N))
        return N if k is None else (k, N)

    # ---------------------------------------------------------------------------------------- inference paths
    def encode(self, seq):
        """Eval-mode representation (is_training=False): rep [n,H] for any n (chunks of MAX_ROWS)."""
        seq = self._enter(seq)
        out = torch.empty((seq.shape[0], self.H), dtype=torch.float32, device=self.device)
        for s, e, _, rep in self._chunks(seq):
            out[s:e] = rep
        return out

    def logits_from_rep(self, rep, max_item, out=None):
        """Dense logits [n, N] = rep . E[1..N]^T  (ADER.py:92)."""
        self._refresh_stream()
        self.sync_table()
        n, N = rep.shape[0], int(max_item)
        if out is None:
            # row stride padded to 16 bytes: the teacher readout of a distilled step streams these rows 16 bytes at a time (k_lx3r);
            # with an odd stride -- max_item is whatever the previous period's catalog was -- it falls back to the slower kernel
            out = torch.empty((n, (N + 3) // 4 * 4), dtype=torch.float32, device=self.device)[:, :N]
        for s in range(0, n, self.MAX_ROWS):
            e = min(n, s + self.MAX_ROWS)
            L.logits_store(self.buf, self._stream(), rep[s:e].contiguous(), self._pp["emb"], self.H, N, out[s:e])
        return out

    def logits(self, seq, max_item):
        return self.logits_from_rep(self.encode(seq), max_item)

    def teacher_logits(self, seq, max_item):
        self._refresh_stream()
        return self.logits(seq, max_item)

    def teacher_rep(self, seq, max_item, lse=False, chunk_rows=None):
        """teacher_logits' small form: TeacherRep(the eval-mode representations [n, H], a copy of table rows 0..max_item, max_item) --
        what the logits [n, max_item] are a pure function of; a distilled step regenerates the rows it needs (ader_teacher_rows).
        lse=True adds the record's lse [n]: the log-sum-exp of every row over its max_item columns, bit for bit ader_row_lse of
        teacher_logits' row -- what the catalog-sharded step needs beside its column window (_train_step_catalog).  The rows pass
        chunk_rows at a time (a multiple of 64; None: as many as keep the workspace under 0.8 GB, at most 1024) through one
        workspace [chunk_rows, max_item padded to 4] and ader_teacher_rows' lse output; nothing of them is kept."""
        self._refresh_stream()
        N = int(max_item)
        _check(1 <= N <= self.item_num, "max_item must be in [1, item_num = %d] (got %d)" % (self.item_num, N))
        ldr = (N + 3) // 4 * 4
        chunk = max(64, min(1024, 200_000_000 // ldr // 64 * 64)) if chunk_rows is None else int(chunk_rows)
        _check(chunk >= 64 and chunk % 64 == 0, "teacher_rep: chunk_rows must be a positive multiple of 64 (got %r)" % (chunk_rows,))
        rep = self.encode(seq)
        trep = TeacherRep(rep, self.param("emb")[:N + 1].detach().clone(), N)
        if not lse:
            return trep
        E, dev, st = rep.shape[0], self.device, self._stream()
        out = torch.empty(E, dtype=torch.float32, device=dev)
        chunk = min(chunk, (max(E, 1) + 63) // 64 * 64)
        rows = torch.empty((chunk, ldr), dtype=torch.float32, device=dev)
        trl, z = torch.empty(chunk, dtype=torch.int32, device=dev), torch.empty(chunk, dtype=torch.float32, device=dev)
        ex = torch.arange(E, dtype=torch.int32, device=dev)
        for s in range(0, E, chunk):
            n = min(chunk, E - s)
            Bk = (n + 63) // 64 * 64
            call("ader_teacher_rows", ptr(trep.rep), ptr(trep.table), ptr(ex[s:]), n, Bk, E, self.H, N, ptr(rows), ldr, ptr(trl), ptr(z),
                 None, st)
            out[s:s + n] = z[:n]
        return TeacherRep(trep.rep, trep.table, N, out)

    def rank_targets(self, seq, pos, max_item, dtype=None, cand_cap=None):
        """0-based rank of pos[b] among items 1..N for every row (Evaluator path, util.py:323-325) -> int32 numpy [n].
        dtype: "f32" (the exact-f32 MFMA kernel) or "x3" (bf16 matrix cores as a filter + exact recheck of the undecided pairs: the same
        ranks, ties included); None: the engine's rank_dtype.  cand_cap: candidate-list entries per chunk of the "x3" path (None: 64 per
        padded row)."""
        dtype = _check_rank_dtype(self.rank_dtype if dtype is None else dtype)
        if dtype == "x3" and rank_x3_supports(self.H):       # (other hidden sizes: the exact kernel, as the flash forward does)
            return self._rank_targets_x3(seq, pos, max_item, cand_cap)
        seq, pos, N = self._enter(seq), self._dev_i32(pos), int(max_item)
        out = torch.empty(seq.shape[0], dtype=torch.int32, device=self.device)
        for s, e, B, rep in self._chunks(seq):
            out[s:e] = L.rank_targets(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, pos[s:e])[:B]
        return out.cpu().numpy()

    def rank_targets_among(self, seq, pos, max_item, candidates=None, exclude_seen=False):
        """rank_targets restricted to a candidate item list, what scores recommend_among: the 0-based rank of pos[b] among
        set(candidates) within [1, max_item], minus the row's seen ids under exclude_seen -> int32 numpy [n].  candidates as
        recommend_among's (candidate_ids: any order, duplicates allowed, every id in [1, item_num]); None: every item of 1..max_item,
        which with exclude_seen=False is rank_targets(dtype="f32").  The target need not be listed and never counts itself, listed or
        seen.  Scores, tie rule (score descending, id ascending) and list are recommend_among's, so for (items, _) =
        recommend_among(seq, k, c, N, exclude_seen=e): rank_targets_among(seq_b, items[b, j], N, c, exclude_seen=e) == j wherever
        items[b, j] > 0.  The list's table rows are gathered inside the kernel (ader_rank_targets_cand, k_rank_cand): the work follows
        len(candidates), not max_item.  Exact-f32 chain whatever rank_dtype says (the x3 filter walks contiguous tiles only).  The list
        is copied to the device once, chunks of MAX_ROWS rows, one device -> host copy."""
        N = self._check_kN("rank_targets_among", int(max_item))
        cand = np.arange(1, N + 1, dtype=np.int32) if candidates is None else candidate_ids(candidates, N, self.item_num)
        seq, pos = self._enter(seq), self._dev_i32(pos)
        cand_d = torch.from_numpy(cand).to(self.device) if cand.shape[0] else None
        out = torch.empty(seq.shape[0], dtype=torch.int32, device=self.device)
        for s, e, B, rep in self._chunks(seq):
            out[s:e] = L.rank_targets_cand(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, pos[s:e], cand_d,
                                           seq[s:e] if exclude_seen else None, self.status)[:B]
        return out.cpu().numpy()

    def _rank_targets_x3(self, seq, pos, max_item, cand_cap):
        """rank_targets on the bf16 matrix cores (ader_rank_targets_x3): per 128-row-padded chunk the x3 filter decides every (row, item)
        whose x3 logit is outside the band tl +- delta, the exact-f32 recheck decides the listed rest; a chunk whose list overflowed is
        ranked again by the exact kernel.  One device -> host copy: ranks + per-chunk (count, max err / delta)."""
        seq, pos = self._enter(seq), self._dev_i32(pos)
        n, N, st, emb = seq.shape[0], int(max_item), self._stream(), self._pp["emb"]
        chunks = [(s, min(n, s + self.MAX_ROWS)) for s in range(0, n, self.MAX_ROWS)]
        res = torch.zeros(n + 2 * len(chunks), dtype=torch.int32, device=self.device)      # ranks | (count, max err / delta) per chunk
        emax = L.rank_emax(self.buf, st, emb, self.item_num, self.H, N) if chunks else None      # once per call, not per chunk
        caps = []
        for c, (s, e, B, rep) in enumerate(self._chunks(seq)):
            caps.append(int(cand_cap) if cand_cap is not None else RANK_X3_CAND_PER_ROW * L.pad_rows(B, 128))
            # (one candidate list for all chunks: their launches are ordered on the stream)
            rk, _ = L.rank_targets_x3(self.buf, st, rep, emb, self.item_num, self.H, N, pos[s:e], emax, caps[c], res[n + 2 * c:])
            res[s:e] = rk[:B]
        host = res.cpu().numpy()
        ranks, diag = host[:n].copy(), host[n:].reshape(-1, 2)
        over = [c for c in range(len(chunks)) if diag[c, 0] > caps[c]]
        # the list overflowed: some undecided pairs were dropped.  The exact kernel ranks the chunk again, on the SAME session forward
        # as this call's: the density of a host batch (which decides "auto" packing, and the packed kernels round differently) is kept
        # for the device slices the inner call sees
        kd, self._step.keep_density = self._step.keep_density, True
        try:
            for c in over:
                s, e = chunks[c]
                ranks[s:e] = self.rank_targets(seq[s:e], pos[s:e], N, dtype="f32")
        finally:
            self._step.keep_density = kd
        self.last_rank_stats = {
            "candidates": int(diag[:, 0].sum()), "pairs": int(n) * N, "overflowed_chunks": len(over),
            "max_err_over_delta": float(diag[:, 1].copy().view(np.float32).max()) if len(chunks) else 0.0}
        return ranks

    def recommend(self, seq, k, max_item=None, exclude_seen=False, dtype=None, band=None):
        """The k best items of 1..max_item for every row, fused with the catalog logits (ader_topk_items): (items int32 [n,k], 1-based;
        scores float32 [n,k]) as numpy.  Order: (score descending, item id ascending) -- the tie rule of rank_targets -- on the very
        float32 logits() returns, so items == stable_argsort(-logits)[:, :k] + 1 and rank_targets(seq_b, items[b, j]) == j.
        exclude_seen removes the non-zero ids of the row's own seq from its candidates (off by default: a repeated item is a legitimate
        target, and the reference's evaluation does not exclude).  Fewer than k candidates: the tail is item 0, score -inf.
        max_item=None: the whole catalog.  Chunks of MAX_ROWS rows, one device -> host copy.
        dtype: "f32" (k_topk_tile on the exact-f32 MFMA chain) or "x3" (bf16 matrix cores as a filter that keeps a superset of every
        row's top-k + exact recheck of the kept pairs: the same bytes, ties included); None: the engine's topk_dtype.  "x3" takes the
        f32 kernels for a hidden size outside k_lx3t's, k > ader_topk_x3_kmax() or a table of 2^31 bytes or more.  band: keys beyond
        k a row's kept set may hold on the "x3" path before the row is handed to the f32 kernels (None: TOPK_X3_BAND).
        recommend_among: the same over a candidate item list."""
        dtype = _check_topk_dtype(self.topk_dtype if dtype is None else dtype)
        k, N = self._check_kN("recommend", max_item, k, call("ader_topk_kmax"))
        band = TOPK_X3_BAND if band is None else int(band)
        _check(0 <= band <= TOPK_X3_BAND, "recommend: band must be in 0..%d (got %d)" % (TOPK_X3_BAND, band))
        if dtype == "x3" and rank_x3_supports(self.H) and k <= call("ader_topk_x3_kmax") and self.item_num * self.H * 4 < 2 ** 31:
            return self._recommend_x3(seq, k, N, exclude_seen, band)
        seq = self._enter(seq)
        res = _Packed(self.device, seq.shape[0], k)
        for s, e, _, rep in self._chunks(seq):
            L.topk_items(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, seq[s:e] if exclude_seen else None, k,
                         *res.rows(s, e))
        return res.cpu()

    def row_stats(self, seq, max_item=None):
        """The model's distribution per row, without the [n, max_item] matrix: (lse, entropy), float32 [n] numpy.  With s = the float32
        logits(seq, max_item)[b]: lse[b] = log sum exp(s) and entropy[b] = -sum p log p in nats, p = exp(s - lse[b]) -- the softmax
        the loss trains, over ALL of 1..max_item (None: the whole catalog).  One catalog walk (ader_row_stats, k_row_stats): per-lane
        (max, sum, weighted sum) states merged in a fixed order, no float atomics, so two calls give the same bits, and they are the
        bits recommend_stats returns for the same rows in the same chunking.  A batch of another size partitions the catalog
        differently (ader_topk_ranges) and may differ in the last bits.  Chunks of MAX_ROWS rows, one device -> host copy."""
        N = self._check_kN("row_stats", max_item)
        seq = self._enter(seq)
        res = torch.empty((2, seq.shape[0]), dtype=torch.float32, device=self.device)       # lse | entropy: one copy back
        for s, e, _, rep in self._chunks(seq):
            L.row_stats(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, res[0, s:e], res[1, s:e])
        host = res.cpu().numpy()
        return host[0], host[1]

    def recommend_stats(self, seq, k, max_item=None, exclude_seen=False):
        """recommend(dtype="f32") with the row's normaliser out of the same catalog walk (ader_topk_items_stats, k_topk_tile_stats):
        (items int32 [n,k], scores float32 [n,k], lse float32 [n], entropy float32 [n]) as numpy.  items / scores are
        recommend(dtype="f32")'s, byte for byte (order, ties, exclude_seen, item 0 / -inf padding); lse / entropy are row_stats',
        bit for bit for the same rows in the same chunking.  They run over ALL of 1..max_item whatever exclude_seen removes from the
        answer: an excluded item keeps its mass, so probs(scores, lse) of an answer need not sum to 1, and a probability means the
        same thing in every call.  k in 1..ader_topk_kmax() (= 64); exact-f32 chain only, whatever topk_dtype says.  Chunks of
        MAX_ROWS rows, one device -> host copy.  (A method of its own: recommend's parameter list is pinned by the tests.)"""
        k, N = self._check_kN("recommend_stats", max_item, k, call("ader_topk_kmax"))
        seq = self._enter(seq)
        self.last_topk_stats = None
        n = seq.shape[0]
        res = _Packed(self.device, n, k, (n, n))                                         # ... | lse bits | entropy bits
        lse, entropy = (x.view(torch.float32) for x in res.extra)
        for s, e, _, rep in self._chunks(seq):
            L.topk_items_stats(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, seq[s:e] if exclude_seen else None, k,
                               *res.rows(s, e), lse[s:e], entropy[s:e])
        items, scores, lse, entropy = res.cpu()
        return items, scores, lse.view(np.float32), entropy.view(np.float32)

    def recommend_among(self, seq, k, candidates, max_item=None, exclude_seen=False, dtype=None):
        """recommend restricted to a candidate item list: candidates is a 1-D integer array / tensor of item ids, shared by all rows
        (candidate_ids: any order, duplicates allowed, every id in [1, item_num]).  A row's candidates are set(candidates) within
        [1, max_item], minus its seen ids under exclude_seen; scores, order, ties and padding are recommend's, so items ==
        stable_argsort(-L)[:, :k] + 1 for L = logits() with every other column at -inf, and with all of 1..max_item the bytes are
        recommend's.  The list's table rows are gathered inside the kernel (ader_topk_items_cand, k_topk_cand): the work follows
        len(candidates), not max_item.  dtype is checked as recommend checks it, but "x3" takes these f32 kernels too (the x3 filter
        walks contiguous tiles only), next to recommend's own cases that fall to f32; last_topk_stats is left None.  (A method of its
        own: recommend's parameter list is pinned by tests/test_topk_x3_host.py; Ader.recommend takes candidates=.)"""
        _check_topk_dtype(self.topk_dtype if dtype is None else dtype)
        k, N = self._check_kN("recommend_among", max_item, k, call("ader_topk_kmax"))
        return self._recommend_cand(seq, k, N, exclude_seen, candidate_ids(candidates, N, self.item_num))

    def _recommend_cand(self, seq, k, N, exclude_seen, cand):
        """recommend over cand, candidate_ids' list: copied to the device once, ader_topk_items_cand per chunk of MAX_ROWS rows, one
        device -> host copy."""
        seq = self._enter(seq)
        self.last_topk_stats = None
        cand_d = torch.from_numpy(cand).to(self.device) if cand.shape[0] else None
        res = _Packed(self.device, seq.shape[0], k)
        for s, e, _, rep in self._chunks(seq):
            L.topk_items_cand(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, cand_d, seq[s:e] if exclude_seen else None, k,
                              *res.rows(s, e), self.status)
        return res.cpu()

    def score_items(self, seq, items, max_item=None):
        """The logits of the listed items, row by row: items is an integer [n, C] array or tensor of item ids (any order, duplicates
        allowed) -> float32 [n, C] numpy aligned with it, the bits of logits(seq, N)[b, items[b, c] - 1]; -inf where items[b, c] <= 0
        or > N = max_item (None: the whole catalog).  What a re-ranking stage asks of the model: the table rows are gathered inside
        the kernel (ader_score_items, k_rowlist), so the work follows n * C and no [n, N] logits are written.  Chunks of MAX_ROWS
        rows, one device -> host copy."""
        N = self._check_kN("score_items", max_item)
        if not isinstance(items, torch.Tensor):
            items = np.asarray(items)
        _check(items.ndim == 2, "score_items: items must be [n, C] (got %d dimensions)" % items.ndim)
        dt = items.dtype
        _check(dt in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) if isinstance(items, torch.Tensor)
               else np.issubdtype(dt, np.integer), "score_items: items must hold integers (got dtype %s)" % (dt,))
        seq = self._enter(seq)
        n, C = seq.shape[0], int(items.shape[1])
        _check(items.shape[0] == n, "score_items: items must have one row per session (got %d for %d)" % (items.shape[0], n))
        out = torch.empty((n, C), dtype=torch.float32, device=self.device)
        if C:
            ids = self._dev_i32(items)
            for s, e, _, rep in self._chunks(seq):
                L.score_items(self._stream(), rep, self._pp["emb"], self.H, N, ids[s:e], out[s:e])
        return out.cpu().numpy()

    def recommend_per_row(self, seq, k, lists, max_item=None, exclude_seen=False):
        """recommend_among with a candidate list of its own for every row: lists as row_candidate_ids takes them (a 2-D integer array
        or tensor with 0 as padding, or a sequence of 1-D integer sequences; any order, duplicates allowed, every id in
        [0, item_num]).  Row b's candidates are set(lists[b]) within [1, max_item], minus its seen ids under exclude_seen; scores,
        order, ties and padding are recommend's, so with all of 1..max_item in every row the bytes are recommend's, and with the same
        list in every row recommend_among's.  The lists' table rows are gathered inside the kernel (ader_topk_items_rows, k_rowlist):
        the work follows the lists' length, not max_item.  Exact-f32 chain; last_topk_stats is left None.  The lists are copied to
        the device once, chunks of MAX_ROWS rows, one device -> host copy."""
        k, N = self._check_kN("recommend_per_row", max_item, k, call("ader_topk_kmax"))
        ids = row_candidate_ids(lists, N, self.item_num)
        seq = self._enter(seq)
        self.last_topk_stats = None
        n = seq.shape[0]
        _check(ids.shape[0] == n, "recommend_per_row: lists must have one row per session (got %d for %d)" % (ids.shape[0], n))
        ids_d = self._dev_i32(ids) if ids.shape[1] else None
        res = _Packed(self.device, n, k)
        for s, e, _, rep in self._chunks(seq):
            L.topk_items_rows(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, ids_d[s:e] if ids.shape[1] else None,
                              seq[s:e] if exclude_seen else None, k, *res.rows(s, e), self.status)
        return res.cpu()

    def rank_targets_per_row(self, seq, pos, max_item, lists, exclude_seen=False):
        """rank_targets_among with a candidate list of its own for every row (lists as recommend_per_row's): the 0-based rank of pos[b]
        among set(lists[b]) within [1, max_item], minus the row's seen ids under exclude_seen -> int32 numpy [n].  The target need not
        be listed and never counts itself, listed or seen; scores and the tie rule (score descending, id ascending) are
        recommend_per_row's, so for (items, _) = recommend_per_row(seq, k, lists, N, e): rank_targets_per_row(seq_b, items[b, j], N,
        lists, e) == j wherever items[b, j] > 0.  With the target plus sampled unseen items as a row's list this is the
        sampled-negative protocol of the SASRec evaluation (data.sample_negatives, Evaluator(negatives=...)).  ader_rank_targets_rows,
        k_rowlist: the work follows the lists' length.  Chunks of MAX_ROWS rows, one device -> host copy."""
        N = self._check_kN("rank_targets_per_row", int(max_item))
        ids = row_candidate_ids(lists, N, self.item_num)
        seq, pos = self._enter(seq), self._dev_i32(pos)
        n = seq.shape[0]
        _check(ids.shape[0] == n, "rank_targets_per_row: lists must have one row per session (got %d for %d)" % (ids.shape[0], n))
        ids_d = self._dev_i32(ids) if ids.shape[1] else None
        out = torch.empty(n, dtype=torch.int32, device=self.device)
        for s, e, B, rep in self._chunks(seq):
            out[s:e] = L.rank_targets_rows(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, pos[s:e],
                                           ids_d[s:e] if ids.shape[1] else None, seq[s:e] if exclude_seen else None, self.status)[:B]
        return out.cpu().numpy()

    def _recommend_x3(self, seq, k, N, exclude_seen, band):
        """recommend on the bf16 matrix cores (ader_topk_items_x3): per 128-row-padded chunk k_lx3t keeps every item whose x3 logit is not
        provably below the row's k-th best, k_topk3_finish rechecks the kept pairs on the exact chain and selects.  One device -> host
        copy of items, scores, status and diag; a chunk with a row whose kept set outgrew k + band keys goes through ader_topk_items on
        the representations kept from this call's forward, and those rows are replaced."""
        seq = self._enter(seq)
        n, st, dev, emb = seq.shape[0], self._stream(), self.device, self._pp["emb"]
        chunks = [(s, min(n, s + self.MAX_ROWS)) for s in range(0, n, self.MAX_ROWS)]
        res = _Packed(dev, n, k, (n, 3 * len(chunks)), zero=True)                        # ... | status | diag
        status, diag = res.extra
        rep_all = torch.empty((n, self.H), dtype=torch.float32, device=dev)
        emax = L.rank_emax(self.buf, st, emb, self.item_num, self.H, N) if chunks else None       # once per call, not per chunk
        for c, (s, e, B, rep) in enumerate(self._chunks(seq, rep_all)):
            stat, _ = L.topk_items_x3(self.buf, st, rep, emb, self.item_num, self.H, N, seq[s:e] if exclude_seen else None, k, band,
                                      emax, *res.rows(s, e), diag[3 * c:])
            status[s:e] = stat[:B]
        h_items, h_scores, h_status, h_diag = res.cpu()
        h_items, h_scores, h_diag = h_items.copy(), h_scores.copy(), h_diag.reshape(-1, 3)
        over = [c for c, (s, e) in enumerate(chunks) if h_status[s:e].any()]
        for c in over:
            s, e = chunks[c]
            fb = _Packed(dev, e - s, k)
            L.topk_items(self.buf, st, rep_all[s:e], emb, self.H, N, seq[s:e] if exclude_seen else None, k, *fb.rows(0, e - s))
            fb_items, fb_scores = fb.cpu()
            rows = np.nonzero(h_status[s:e])[0]
            h_items[s + rows], h_scores[s + rows] = fb_items[rows], fb_scores[rows]
        self.last_topk_stats = {
            "kept_pairs": int(h_diag[:, 0].sum()), "rows": int(n), "overflowed_rows": int(np.count_nonzero(h_status)),
            "fallback_chunks": len(over),
            "max_err_over_delta": float(h_diag[:, 2].copy().view(np.float32).max()) if len(chunks) else 0.0}
        return h_items, h_scores

    def recommend_wide(self, seq, k, max_item=None, exclude_seen=False, cap=None):
        """recommend's contract for wide answers, 1 <= k <= ader_topk_wide_kmax() (= 1024): (items int32 [n,k], scores float32 [n,k]) as
        numpy, items == stable_argsort(-logits)[:, :k] + 1 on the very float32 logits() returns, order (score descending, item id
        ascending), exclude_seen and the item 0 / -inf padding as recommend's; for k <= 64 the bytes are recommend(dtype="f32")'s.
        Slab and select (ader_topk_items_wide, csrc/topk.hip): per row a list of cap keys in global memory (cap: a multiple of 64
        in [k + 64, ader_topk_wide_cap()]; None: the largest, 4096), cut to its exact best k between slabs of the catalog walk; no
        [n, max_item] logits are written.  Chunks of MAX_ROWS rows, one device -> host copy of items, scores, status and diag.  A row
        whose list overflowed between two selects (scores trending upwards with the item id) is recomputed exactly, and slowly: dense
        logits of those rows in groups under 256 MB, the seen columns at -inf, a stable descending sort, the same padding.
        last_topk_stats: slabs (per chunk), rows, max_list (the largest list a select after slab 0 met), overflowed_rows,
        fallback_rows."""
        capmax = call("ader_topk_wide_cap")
        k, N = self._check_kN("recommend_wide", max_item, k, call("ader_topk_wide_kmax"))
        cap = capmax if cap is None else int(cap)
        _check(cap % 64 == 0 and k + 64 <= cap <= capmax,
               "recommend_wide: cap must be a multiple of 64 in [k + 64 = %d, %d] (got %d)" % (k + 64, capmax, cap))
        seq = self._enter(seq)
        n, dev = seq.shape[0], self.device
        n_chunks = (n + self.MAX_ROWS - 1) // self.MAX_ROWS
        res = _Packed(dev, n, k, (n, 2 * n_chunks), zero=True)                           # ... | status | diag
        status, diag = res.extra
        rep_all = torch.empty((n, self.H), dtype=torch.float32, device=dev)
        for c, (s, e, B, rep) in enumerate(self._chunks(seq, rep_all)):
            stat, _ = L.topk_items_wide(self.buf, self._stream(), rep, self._pp["emb"], self.H, N, seq[s:e] if exclude_seen else None, k,
                                        cap, *res.rows(s, e), diag[2 * c:])
            status[s:e] = stat[:B]
        h_items, h_scores, h_status, h_diag = res.cpu()
        h_items, h_scores, h_diag = h_items.copy(), h_scores.copy(), h_diag.reshape(-1, 2)
        over = np.nonzero(h_status)[0]
        group = max(1, 64_000_000 // ((N + 3) // 4 * 4))          # rows whose dense logits stay under 256 MB
        m = min(k, N)
        for g in range(0, len(over), group):
            rows = torch.from_numpy(over[g:g + group]).to(dev)
            lg = self.logits_from_rep(rep_all[rows], N).contiguous()
            if exclude_seen:
                ids = seq[rows].long()
                ids = torch.where(ids <= N, ids, torch.zeros_like(ids))              # column 0 = "no id" (and ids above N)
                lg = torch.cat([torch.zeros((lg.shape[0], 1), dtype=lg.dtype, device=dev), lg], 1)
                lg.scatter_(1, ids, float("-inf"))
                lg = lg[:, 1:]
            v, i = torch.sort(lg, dim=1, stable=True, descending=True)
            v, i = v[:, :m].cpu().numpy(), (i[:, :m] + 1).to(torch.int32).cpu().numpy()
            i[np.isneginf(v)] = 0
            h_items[over[g:g + group]], h_scores[over[g:g + group]] = 0, -np.inf
            h_items[over[g:g + group], :m], h_scores[over[g:g + group], :m] = i, v
        self.last_topk_stats = {
            "slabs": int(call("ader_topk_wide_slabs", N, k, cap, None, 0)), "rows": int(n),
            "max_list": int(h_diag[:, 0].max()) if n_chunks else 0, "overflowed_rows": int(len(over)), "fallback_rows": int(len(over))}
        return h_items, h_scores

    def row_losses(self, seq, pos, max_item):
        """Per-row cross entropy -log softmax(logits)[label] in eval mode (the quantity the reference's `loss` exemplar selector
        means to rank by, util.py:463-495; its graph fetches the batch MEAN, see ExemplarGenerator.loss_selection) -> float32 [n]
        device tensor.  Exact-f32 logit kernels, chunks of MAX_ROWS rows."""
        seq, pos, N = self._enter(seq), self._dev_i32(pos), int(max_item)
        out = torch.empty(seq.shape[0], dtype=torch.float32, device=self.device)
        st = self._stream()
        parts = call("ader_logits_parts", N)
        scr = torch.empty(1, dtype=torch.float32, device=self.device)
        for s, e, B, rep in self._chunks(seq):
            Bp, ri = self._rowinfo(B, pos[s:e].contiguous(), B, None, None, N, 0, 1.0, 0.0, None, tag="rl_")
            part = self.buf("lg_part", (parts * Bp * 3,))
            lse, rowloss = self.buf("rl_lse", (Bp,)), self.buf("rl_rowloss", (Bp,))
            call("ader_logits_loss_fwd", ptr(rep), self._pp["emb"], B, Bp, self.H, N, *ri, ptr(part), ptr(lse), ptr(rowloss),
                 ptr(scr), st)
            out[s:e] = rowloss[:B]
        return out

    def herding_select(self, seq_rows, offs, quota, max_item):
        """Segmented herding over label groups (util.py:436-461).  seq_rows [n,T] candidates in group order, offs [G+1],
        quota [G] = min(m, n_g).  Returns (sel [n] local indices per group span, sel_cnt [G]) as numpy."""
        self._refresh_stream()
        from ..exemplar import herding_max_steps
        rep = self.encode(seq_rows)
        n, G = rep.shape[0], len(quota)
        seg = torch.as_tensor(np.asarray(offs, dtype=np.int64)).to(self.device)
        q = torch.as_tensor(np.asarray(quota, dtype=np.int32)).to(self.device)
        ms = torch.as_tensor(np.array([herding_max_steps(int(m)) for m in quota], dtype=np.int32)).to(self.device)
        D = torch.empty(n * self.H + G + 64, dtype=torch.float32, device=self.device)     # normalised columns + the device-built work list
        chosen = torch.empty(max(n, 1), dtype=torch.uint8, device=self.device)
        sel = torch.zeros(max(n, 1), dtype=torch.int32, device=self.device)
        cnt = torch.zeros(max(G, 1), dtype=torch.int32, device=self.device)
        call("ader_herding_select", ptr(rep), ptr(seg), ptr(q), ptr(ms), G, n, self.H, ptr(D), ptr(chosen), ptr(sel), ptr(cnt),
             None, self._stream())
        return sel.cpu().numpy().astype(np.int64), cnt.cpu().numpy()
