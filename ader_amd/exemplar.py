"""Exemplar selection: the MI355X build's counterpart of the reference's ``ExemplarGenerator``
(util.py:353-461: ``__init__`` grouping + multinomial quotas, ``herding``, ``herding_selection``).

The reference issues one ``sess.run`` per distinct label (~17k per DIGINETICA period, util.py:447-455)
and runs the greedy herding loop in numpy on the host.  Here all candidates go through ONE batched
eval-mode encode on the GPU, the herding loop runs as one segmented HIP kernel launch over all label
groups (csrc/herding.hip), and the teacher logits of the selected rows stay on the device as one
[E, N] tensor instead of Python float lists (util.py:433) -- or, in the "rep" form, as what those logits are a
function of: the teacher's representations [E, H] and a copy of the item table (engine.TeacherRep).
"""
from collections import defaultdict

import numpy as np

from . import data as _data


def draw_quotas(groups, exemplar_size, disable_m, max_item):
    """Per-item exemplar quotas (util.py:393-399): multinomial(m, freq/sum(freq)) on numpy's legacy
    global RNG; `disable_m` (--equal_exemplar) uses uniform probabilities over all max_item items."""
    item_count = np.zeros(max_item)
    if isinstance(groups, _data.LabelGroups):
        item_count[groups.labels - 1] += groups.sizes
    else:
        for label, rows in groups.items():
            item_count[label - 1] += len(rows)
    if disable_m:
        item_count = np.ones_like(item_count)
    item_prob = item_count / item_count.sum()
    return np.int32(np.random.multinomial(n=exemplar_size, pvals=item_prob, size=1)[0])


def herding_max_steps(m):
    """Loop bound of `while ... and step_t < 1.1 * m` (util.py:425), evaluated in float64 as Python does."""
    lim = 1.1 * float(m)
    k = int(lim)
    while k < lim:
        k += 1
    return k


class _RepRows:
    """`logits[i]` of a store in the rep form: the teacher row of exemplar i, computed when somebody asks (in chunks of 256 rows)."""

    def __init__(self, trep):
        self.trep, self._lo, self._chunk = trep, -1, None

    def __len__(self):
        return len(self.trep)

    def __getitem__(self, i):
        i = int(i)
        if not 0 <= i < len(self.trep):
            raise IndexError(i)
        lo = i // 256 * 256
        if lo != self._lo:
            self._chunk, self._lo = self.trep.rows(np.arange(lo, min(lo + 256, len(self.trep)))), lo
        return self._chunk[i - lo]


class ExemplarStore:
    """Selected exemplars of one period: sessions as [E, maxlen+1] int32 rows (inputs ‖ label) and their teacher -- `teacher` is
    either the logits [E, N] (float32, device tensor when produced by the GPU path) or a TeacherRep (representations [E, H] + the
    table snapshot [N+1, H]): what a distilled step takes as `teacher=`."""

    def __init__(self, rows, teacher, max_item):
        self.rows = rows
        self.teacher = teacher
        self.max_item = max_item

    @property
    def form(self):
        return "rep" if _is_rep(self.teacher) else "logits"

    @property
    def logits(self):
        """Teacher logits by exemplar: the [E, N] tensor, or (rep form) a view that computes a row when it is indexed."""
        return _RepRows(self.teacher) if _is_rep(self.teacher) else self.teacher

    @logits.setter
    def logits(self, value):
        self.teacher = value

    def tensors(self):
        """Every tensor / array the store holds."""
        if not _is_rep(self.teacher):
            return [self.rows, self.teacher]
        t = self.teacher
        return [self.rows, t.rep, t.table] + ([t.lse] if getattr(t, "lse", None) is not None else [])

    def __len__(self):
        return int(self.rows.shape[0])

    def sessions(self):
        """Sessions in the reference's stored form: non-zero inputs followed by the label (util.py:433) -- as a PackedSessions (a
        sequence of lists held as arrays: what main.py hands on as the next period's exemplar candidates)."""
        return _data.PackedSessions.from_rows(self.rows)

    # The reference keeps the exemplars in memory only (main.py:312): a crash loses them.  Here they can be written next to
    # the period's checkpoint and read back (rows + teacher logits + the catalog size they were computed for).
    def save(self, path):
        import torch
        rows = torch.as_tensor(np.ascontiguousarray(np.asarray(self.rows), dtype=np.int32))
        if _is_rep(self.teacher):
            t = self.teacher
            d = {"rows": rows, "rep": t.rep.detach().cpu().contiguous(), "table": t.table.detach().cpu().contiguous(),
                 "Np": int(t.Np), "max_item": int(self.max_item)}
            if getattr(t, "lse", None) is not None:         # (the rows' log-sum-exps: a record taken for the catalog-sharded step)
                d["lse"] = t.lse.detach().cpu().contiguous()
            torch.save(d, path)
            return path
        lg = self.logits.detach().cpu().contiguous() if hasattr(self.logits, "detach") else torch.as_tensor(np.asarray(self.logits))
        torch.save({"rows": rows, "logits": lg, "max_item": int(self.max_item)}, path)
        return path

    @classmethod
    def load(cls, path, device=None):
        import torch
        d = torch.load(path, weights_only=True)        # tensors and plain numbers only: nothing is unpickled
        if "rep" in d:
            from .engine.common import TeacherRep
            t = TeacherRep(d["rep"], d["table"], int(d["Np"]), d.get("lse"))
            return cls(d["rows"].numpy(), t if device is None else t.to(device), int(d["max_item"]))
        lg = d["logits"]
        if device is not None:          # on the device the rows keep the 16-byte aligned stride Engine.teacher_logits gives them
            pad = torch.empty((lg.shape[0], (lg.shape[1] + 3) // 4 * 4), dtype=lg.dtype, device=device)[:, :lg.shape[1]]
            pad.copy_(lg)
            lg = pad
        return cls(d["rows"].numpy(), lg, int(d["max_item"]))

    def by_label(self):
        """{item: [[session, logits_row], ...]} -- the reference's `fast_exemplar` view (util.py:433), rows in store order."""
        out = defaultdict(list)
        logits = self.logits            # (rep form: ONE row view, so that its chunk of computed rows is reused)
        for i, r in enumerate(np.asarray(self.rows)):
            out[int(r[-1])].append([r[r != 0].tolist(), logits[i]])
        return out


def _is_rep(teacher):
    return hasattr(teacher, "rep") and hasattr(teacher, "table")          # (engine.TeacherRep, without importing the engine here)


class ExemplarGenerator:
    """Same constructor arguments as the reference (util.py:366-374); teacher_form: "logits" = the store keeps the teacher logits
    [E, N] (util.py:433), "rep" = the teacher's representations and a table snapshot (engine.TeacherRep)."""

    def __init__(self, data, exemplar_size, disable_m, batch_size, maxlen, dropout_rate, max_item, shard=(0, 1), teacher_form="logits"):
        if teacher_form not in ("logits", "rep"):
            raise ValueError("teacher_form must be 'logits' or 'rep' (got %r)" % (teacher_form,))
        self.teacher_form = teacher_form
        self.shard = shard          # (rank, world): label groups are independent herding units
        self._exemplars, self._view = defaultdict(list), None
        self.m = exemplar_size
        self.max_item = max_item
        self.maxlen = maxlen
        self.dropout_rate = dropout_rate
        self.sess_by_item = _data.group_by_label(data, batch_size, maxlen)
        self.item_count = draw_quotas(self.sess_by_item, exemplar_size, disable_m, max_item)
        self.store = None

    @property
    def exemplars(self):
        """{item: [[session, logits_row], ...]} -- the reference's `fast_exemplar` (util.py:433), built from the store when somebody
        asks for it (main.py hands the store itself to the next period: ~30k small lists per period are not built to be re-packed)."""
        if self._view is not None:
            labels, counts, sel_rows, logits = self._view
            self._view = None
            p = 0
            for label, c in zip(labels, counts):
                if c or label in self._keep_empty:
                    self._exemplars[label] = [[r[r != 0].tolist(), logits[p + i]] for i, r in enumerate(sel_rows[p:p + c])]
                p += c
        return self._exemplars

    def _set_view(self, labels, counts, sel_rows, logits, keep_empty=False):
        self._keep_empty = set(labels) if keep_empty else set()
        self._view = (list(labels), [int(c) for c in counts], sel_rows, logits)

    def _make_store(self, model, sel_rows):
        """self.store <- the selected rows with their teacher in the form asked for; returns the logits-by-exemplar of the views."""
        seq = sel_rows[:, :self.maxlen]
        eng = model.engine
        if self.teacher_form == "rep":
            # an engine that will step catalog-sharded reads COLUMNS of the regenerated rows: it needs the rows' log-sum-exps stored
            sharded = getattr(eng, "dp_world", 1) > 1 and getattr(eng, "dp_mode", None) == "catalog"
            teacher = eng.teacher_rep(seq, self.max_item, lse=True) if sharded else eng.teacher_rep(seq, self.max_item)
        else:
            teacher = eng.teacher_logits(seq, self.max_item)
        self.store = ExemplarStore(sel_rows, teacher, self.max_item)
        return self.store.logits

    def _segments(self):
        g = self.sess_by_item
        labels, offs, rows = g.labels.tolist(), g.offs, g.rows
        quota = np.minimum(self.item_count[g.labels - 1].astype(np.int64), g.sizes).astype(np.int32)
        return labels, offs, quota, rows

    def herding_selection(self, sess, model):
        """Select exemplars by herding (util.py:436-461).  `model` is an ader_amd.model.Ader; `sess` is
        accepted for call-surface compatibility.  Returns the number of exemplars saved."""
        labels, offs, quota, rows = self._segments()
        rank, world = self.shard
        if world == 1:
            sel_idx, sel_cnt = model.engine.herding_select(rows[:, :self.maxlen], offs, quota, self.max_item)
        else:
            # each rank selects inside its contiguous chunk of label groups; the per-group index lists are exchanged
            # (quotas were drawn from the same RNG stream on every rank, util.py:398)
            from . import dist as _dist
            chunks = _dist.split_groups(np.diff(offs).tolist(), world)
            g0, g1 = chunks[rank]
            r0, r1 = int(offs[g0]), int(offs[g1])
            if g1 > g0:
                li, lc = model.engine.herding_select(rows[r0:r1, :self.maxlen], offs[g0:g1 + 1] - r0, quota[g0:g1],
                                                     self.max_item)
            else:
                li, lc = np.zeros(0, np.int64), np.zeros(0, np.int32)
            parts = _dist.gather_lists((np.asarray(li), np.asarray(lc)), world)
            sel_idx = np.concatenate([np.asarray(p[0]) for p in parts])
            sel_cnt = np.concatenate([np.asarray(p[1]) for p in parts])
        keep = []
        for g, label in enumerate(labels):
            c = int(sel_cnt[g])
            ids = sel_idx[offs[g]:offs[g] + c] + offs[g]
            keep.append(ids)
        keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        sel_rows = rows[keep]
        logits = self._make_store(model, sel_rows)
        # reference-shaped view {item: [[session, logits_row], ...]} (logits rows are views of the store): built on demand
        self._set_view(labels, sel_cnt[:len(labels)], sel_rows, logits, keep_empty=True)
        return int(len(keep))

    def loss_selection(self, sess, model, first_only=False):
        """Exemplars with the SMALLEST loss per label (util.py:463-495), ranking by the per-row cross entropy.

        first_only (driver flag `--selection loss_ref`): what the reference's code EXECUTES rather than what it documents -- the first
        candidate of every label with a quota >= 1 (see below): the exemplar set of the poster's `loss` columns, if the published
        code produced them.

        The reference fetches `model.loss` -- the batch MEAN, a scalar (ADER.py:93) -- so its `loss.argsort()[:m]` sees a 0-d array,
        yields [0] and always keeps just the FIRST candidate of every label.  This implementation does
        what the method documents ("selects exemplars by ranking loss"): one batched eval-mode pass gives every candidate's own
        -log softmax(logits)[label]; per label the min(m, n) rows of smallest loss are kept, ties by candidate order (stable
        argsort, as numpy's on equal keys).  Labels with quota 0 are skipped (`if m < 0.5: continue`, util.py:481)."""
        labels, offs, quota, rows = self._segments()
        loss = model.engine.row_losses(rows[:, :self.maxlen], rows[:, self.maxlen], self.max_item).cpu().numpy()
        keep, counts = [], []
        for g, label in enumerate(labels):
            n = int(offs[g + 1] - offs[g])
            m = int(self.item_count[label - 1])
            c = 0
            if m >= 1:
                ids = (np.zeros(1, np.int64) if first_only else
                       np.argsort(loss[offs[g]:offs[g + 1]], kind="stable")[:min(m, n)])
                keep.append(ids + offs[g])
                c = len(ids)
            counts.append(c)
        keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        sel_rows = rows[keep]
        logits = self._make_store(model, sel_rows)
        self._set_view(labels, counts, sel_rows, logits)
        return int(len(keep))

    def randomly_selection(self, sess, model):
        """Random exemplars per label (util.py:497-522): np.random.choice without replacement, in group order."""
        labels, offs, quota, rows = self._segments()
        keep, counts = [], []
        for g, label in enumerate(labels):
            n = int(offs[g + 1] - offs[g])
            m = int(self.item_count[label - 1])
            c = 0
            if m > 0:
                ids = np.random.choice(n, min(m, n), replace=False)
                keep.append(ids + offs[g])
                c = len(ids)
            counts.append(c)
        keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
        sel_rows = rows[keep]
        logits = self._make_store(model, sel_rows)
        self._set_view(labels, counts, sel_rows, logits)
        return int(len(keep))
