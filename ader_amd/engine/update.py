"""Optimiser side of the step (ADER.py:96, main.py:233-256): sparse lists, fused table update + Adam, train_step dispatch, EWC."""
import numpy as np
import torch

from .._lib import call, ptr
from .common import IN_LR, StepF, issue_table_job


class _Update:
    def _lr_t(self, lr):
        """Adam's step size lr * sqrt(1 - beta2^t) / (1 - beta1^t) in float32 (tf.train.AdamOptimizer; the one launcher argument that
        changes every step: marked for the launch-plan recorder)."""
        return StepF(np.float32(lr) * np.sqrt(np.float32(1) - self.b2p) / (np.float32(1) - self.b1p), IN_LR)

    def _advance_adam(self):
        self.refresh_weights()
        self._advance_step()

    def _advance_step(self):      # the host half of an optimiser step (also behind a replayed plan)
        self.b1p = np.float32(self.b1p * np.float32(self.beta1))
        self.b2p = np.float32(self.b2p * np.float32(self.beta2))
        self.global_step += 1

    def adam(self, lr):
        """tf.train.AdamOptimizer step on every variable (dense, incl. the whole table; ADER.py:96)."""
        self._refresh_stream()
        self._gather_if_sharded()
        with self._sec("adam"):
            call("ader_adam_step", ptr(self.theta), ptr(self.adam_m), ptr(self.adam_v), ptr(self.grad), self.P, self._lr_t(lr),
                 self.beta1, self.beta2, self.eps, ptr(self.shadow), self.V * self.H, self.H, self._stream())
        self._advance_adam()

    def _sparse_lists(self, seq, lab, N):
        """Bucketed lists of the sparse table-gradient terms (input positions, one-hot targets) for the fused table update:
        (ids, positions, bucket starts) x 2 -- buckets of 64 ids in id order, inside a bucket in position order, so the
        contributions to a table row are added in position order (deterministic) -- and, in x3 mode, the per-tile records of the
        64-row kernel.  Built by ader_sparse_lists (csrc/index_prep.hip) into persistent buffers."""
        seq, lab = seq.reshape(-1), lab.reshape(-1)
        if seq.dtype != torch.int32:
            seq = seq.to(torch.int32)
        if lab.dtype != torch.int32:
            lab = lab.to(torch.int32)
        n_sp, n_tg = seq.numel(), lab.numel()
        nb1 = call("ader_sparse_lists_starts", N)
        i32 = torch.int32
        ids, order = self.buf("sl_ids", (n_sp,), i32), self.buf("sl_rows", (n_sp,), i32)
        tids, torder = self.buf("sl_tids", (n_tg,), i32), self.buf("sl_trows", (n_tg,), i32)
        sp_start, tg_start = self.buf("sl_sps", (nb1,), i32), self.buf("sl_tgs", (nb1,), i32)
        scratch = self.buf("sl_scratch", (call("ader_sparse_lists_scratch_n", n_sp, n_tg, N),), i32)
        meta = None
        if self.lx3 or self.bf16_update == "resident":        # per-tile list records of the 64-row update kernel (table_update.hip)
            meta = self.buf("sl_meta", (call("ader_tab_meta_ints", N),), torch.int32)
        # (lists + records: ONE launch on the catalogs of the shipped datasets, the chain of launches on large ones)
        call("ader_sparse_lists_meta", ptr(seq.contiguous()), n_sp, ptr(lab.contiguous()), n_tg, N, ptr(scratch), ptr(ids), ptr(order),
             ptr(sp_start), ptr(tids), ptr(torder), ptr(tg_start), ptr(meta), self._stream())
        return ids, order, sp_start, tids, torder, tg_start, meta

    def _lists_async(self, seq, lab, N):
        main, sx = self._main, self._step
        # flat, contiguous int32 copies are made HERE, by torch on the main stream and before the side stream is told to wait for it:
        # a strided view (the catalog-sharded step passes ids_g[:, :n_pos]) would otherwise be materialised inside _sparse_lists --
        # a torch kernel on the main stream that the list kernels on the side stream do not wait for
        seq, lab = seq.reshape(-1).to(torch.int32).contiguous(), lab.reshape(-1).to(torch.int32).contiguous()
        self._edge(self._side_lane(), main)      # inputs ready; also orders reuse of last step's list memory after its reader
        with self._OnStream(self, self._side):
            sx.lists = self._sparse_lists(seq, lab, N)
            if sx.pending_loss is not None:
                # the loss scalar feeds nothing in this step: its (single-workgroup) sum rides behind the lists on the side lane -- the
                # row losses are complete (the edge above follows the logit forward) -- instead of heading the side lane's chain beside
                # the table update, which at the shipped datasets' shapes ends a few microseconds after the update does
                self._settle_loss()
        sx.lists_seq = (seq, lab)

    def _lists_wait(self):
        out, self._step.lists = self._step.lists, None
        self._edge(self._main, self._side)       # (the lists live in persistent workspace buffers: no record_stream needed)
        return out

    def _table_update(self, job, lists, lr_t, tile_begin=0, tile_count=-1, bf16="sh"):
        """issue_table_job for this engine's table, on the current stream (the data-parallel updates always take the shadow kernel).  x3:
        the operand rows go as the LDS images k_tab32x3 streams by LDS-DMA, cut here unless this step's logit forward did (img_ready)."""
        img = self.buf("lbf_rep_img", (call("ader_x3_rep_image_bytes", job.Bp),), torch.uint8, zero=True) if self.lx3 else None
        if self.lx3 and not self._step.img_ready:
            call("ader_x3_rep_image", ptr(job.hi), ptr(job.lo), job.Bp, ptr(img), self._stream())
        self._step.img_ready = False
        issue_table_job(job, lists, (self.theta, self.adam_m, self.adam_v), self.item_num, self.H, self.shadow, img, lr_t, self.beta1,
                        self.beta2, self.eps, self._stream(), tile_begin, tile_count, bf16)

    def _small_adam(self, lr_t):
        """Adam on every parameter behind the item table: the flat kernel on the tail of the buffer, on the current stream."""
        span = self.layout["pos"][0]
        with self._sec("adam"):
            call("ader_adam_step", self.theta.data_ptr() + 4 * span, self.adam_m.data_ptr() + 4 * span,
                 self.adam_v.data_ptr() + 4 * span, self.grad.data_ptr() + 4 * span, self.P - span, lr_t, self.beta1,
                 self.beta2, self.eps, None, 0, self.H, self._stream())

    def _fused_table_adam(self, lr):
        """Table rows 1..N: gradient GEMM + sparse terms + Adam in one pass (ader_lbf_bwd_adam); all other parameters:
        the flat Adam kernel on the tail of the buffer.  Rows 0 and > N have zero gradient and zero Adam state (the
        catalog only grows), so leaving them untouched equals the dense update."""
        sx = self._step
        lr_t = self._lr_t(lr)
        lists = self._lists_wait()

        def small_update():     # everything that feeds / is the update of the non-table parameters
            if sx.pending_loss is not None:
                self._settle_loss()
            self._flush_late()
            self._atb_flush()
            self._small_adam(lr_t)
            self._advance_adam()

        main = self._main
        overlap = bool(sx.late or sx.atb_q) and self.late_side_stream
        if overlap:
            # weight-gradient products, LayerNorm / positional reductions, small Adam and the bf16 weight planes are compute /
            # latency bound and independent of the table: a side stream runs them under the HBM-bound table update.  The side
            # stream's wait is placed HERE (behind the backward chain), the update is ENQUEUED FIRST and the small launches after
            # it: on the small catalogs of the shipped datasets the host is only a launch or two ahead of the GPU, and with the eight
            # small launches enqueued first the update reached the queue 100 us after the backward chain had finished
            # (profiles/r5_packed/timeline_cfgY_update_late.txt)
            self._edge(self._side_lane(), main)
        with self._sec("logits_bwd_adam"):
            self._table_update(sx.deferred, lists, lr_t, bf16=self.bf16_update)
        if overlap:
            with self._OnStream(self, self._side):
                small_update()
            self._edge(main, self._side)
        else:
            small_update()
        sx.deferred = None

    def train_step(self, seq, pos, max_item, lr, **kw):
        """One `sess.run(train_op)` (main.py:233-256): forward, loss, backward, [gradient exchange], Adam.
        Returns the loss as a 1-element device tensor (no host sync)."""
        self._refresh_stream()
        self._check_teacher(kw.get("teacher"))
        self._begin_step()
        self._in_step = True
        try:
            out = self._native_step(seq, pos, max_item, lr, kw)        # one C call per step when a launch plan exists (plan.py)
            return out if out is not None else self._train_step(seq, pos, max_item, lr, **kw)
        finally:
            self._in_step = False

    def _train_step(self, seq, pos, max_item, lr, **kw):
        if (self.dp_world > 1 and self.dp_mode == "catalog" and (self.shadow is not None or self.lx3) and self.seq_fused
                and kw.get("ex_pos") is None and (kw.get("teacher") is None or self.lx3)):
            return self._train_step_catalog(seq, pos, max_item, lr, **kw)
        kw.pop("ids_host", None)           # (host-side knowledge of the global batch: only the packed catalog exchange uses it)
        kw.pop("pack_counts", None)
        self.sync_table()
        sharded = self.dp_world > 1 and self.dp_sharded and self.shadow is not None      # (x3 / f32 logits: dense exchange)
        fuse = self.fuse_adam and (self.grad_hook is None or sharded)
        if self.ewc is not None and self.ewc["lam"] != 0.0:
            fuse, sharded = False, False         # the penalty's gradient lives in the dense gradient buffer
        loss = self.loss_and_grad(seq, pos, max_item, _defer_table=fuse, **kw)
        if self._step.deferred is not None:
            if sharded:
                self._fused_table_adam_sharded(lr)
            else:
                self._fused_table_adam(lr)
            return loss
        if self.grad_hook is not None:
            with self._sec("grad_exchange"):
                self.grad_hook(self)
        if self.ewc is not None and self.ewc["lam"] != 0.0:
            # loss += lambda/2 sum F (theta - theta_prev)^2 and its gradient (EWC.py:121-124); every rank holds the same F / prev
            call("ader_ewc_penalty", ptr(self.theta), ptr(self.ewc["prev"]), ptr(self.ewc["F"]), ptr(self.grad), self.P,
                 float(self.ewc["lam"]), ptr(self.buf("ewc_part", (1024,))), ptr(self.loss), self._stream())
        self.adam(lr)
        return loss

    # ---------------------------------------------------------------------------------------- EWC baseline (EWC.py:115-164)
    def ewc_snapshot(self):
        """variables_prev = sess.run(model.variables) (main.py:260,321): the parameters the penalty pulls towards."""
        self._refresh_stream()
        if self.ewc is None:
            self.ewc = {"F": torch.zeros(self.P, dtype=torch.float32, device=self.device), "lam": 0.0}
        self.ewc["prev"] = self.theta.detach().clone()

    def compute_fisher(self, seq, pos, max_item):
        """Diagonal Fisher information of EWC.py:126-164: the mean over the n given sub-sequences of the SQUARED per-sample
        gradient of the eval-mode cross entropy (batch of one, dropout off) w.r.t. every parameter -> self.ewc["F"] (flat, the
        parameter layout).  One forward / backward per sample like the reference (n <= --ewc_sample_num = 1000).
        Deviation, on purpose: the reference densifies the position table's IndexedSlices gradient with `dense[idx] = value`
        (EWC.py:153-157), an ASSIGNMENT -- for a row that occurs more than once in a sample only the last slice survives -- whereas
        the SUMMED gradient is squared here (the mathematical Fisher diagonal).  Only rows repeated inside one sample differ
        (tests/test_gpu_extras.py pins the summed semantics against the oracle)."""
        self._refresh_stream()
        self.sync_table()
        if self.ewc is None:
            self.ewc_snapshot()
        seq, pos = self._seq_in(seq), self._dev_i32(pos)
        n = seq.shape[0]
        F = self.ewc["F"]
        F.zero_()
        hook, early = self.grad_hook, self.grad_early_hook
        self.grad_hook = self.grad_early_hook = None
        step = self.global_step
        try:
            for i in range(n):
                # (loss_and_grad overwrites only the table rows <= max_item; rows above were never touched and are zero)
                self.loss_and_grad(seq[i:i + 1], pos[i:i + 1], max_item, rate=0.0)
                call("ader_sq_accum", ptr(self.grad), ptr(F), self.P, 1.0 / n, self._stream())
        finally:
            self.grad_hook, self.grad_early_hook = hook, early
            self.global_step = step
        return F
