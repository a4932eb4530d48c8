"""Forward/backward orchestration of the WavJEPA pre-training step on one MI355X.

This is the host side of the hot path: a fixed sequence of C-ABI kernel launches over a pre-allocated activation
arena (no autograd graph, no allocator traffic in the step, no host synchronisation), mirroring
reference wavjepa/jepa.py:365-419 (forward), :230-270 (teacher targets), :335-362 (loss) and the implicit autograd
backward of those ops.  Activations are token-major bf16/fp32 buffers sized once per batch size; the residual
stream is fp32 and every GEMM operand is bf16, exactly the dtype flow bf16 autocast produces on the reference.

JepaEngine is encoder_engine.EncoderEngine (the front-end and the student stack, forward and backward, the arena, the side stream)
with a second trainable stack, the predictor ("dec"), and what the JEPA objective adds: the mask plan (mask_plan.py), the EMA
teacher and its targets, the masked loss and the collapse monitor.
"""
from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import torch

from . import ops
from .conv_frontend import ConvFrontend, ConvLayerParams, _empty, conv_active_rows, conv_geometry  # noqa: F401  (re-exported)
from .encoder_engine import EncoderEngine, EngineConfig, _layer_ptrs  # noqa: F401  (re-exported)
from .freeze import BackwardPlan
from .mask_plan import MaskPlan, make_mask_plan  # noqa: F401  (re-exported)
from .params import FlatParams
from .upload import _UPLOAD_STREAMS, _upload_stream, pack_upload  # noqa: F401  (re-exported)


class JepaEngine(EncoderEngine):
    BW_RING = dict(EncoderEngine.BW_RING, dec=(2, 1))
    MODULE = dict(EncoderEngine.MODULE, dec="decoder")

    def __init__(self, cfg: EngineConfig, flat: FlatParams, pos_enc: torch.Tensor, pos_dec: torch.Tensor):
        if cfg.loss_kind not in ops.LOSS_KINDS:
            raise ValueError(f"loss_kind {cfg.loss_kind!r}: one of {sorted(ops.LOSS_KINDS)}")
        super().__init__(cfg, flat, pos_enc)
        self.pos_dec = pos_dec.reshape(-1, cfg.d_dec).contiguous().float().to(self.dev)
        self._pos_src.append((self.pos_dec, pos_dec))
        self.G = 0              # target groups per clip of the arena (taken from the mask plan)
        self.plan: Optional[MaskPlan] = None       # of the forward being run
        # visible-token (ragged) execution of the student and the predictor; WJ_RAGGED=0 keeps the reference's dense
        # key-masked shapes (identical loss and gradients, ~2x the work)
        self.ragged = os.environ.get("WJ_RAGGED", "1") != "0"
        self.ragged_step = False
        # last predictor layer: after its attention only the target rows go on (WJ_TRIM_TAIL=0: every visible row)
        self.trim_tail = os.environ.get("WJ_TRIM_TAIL", "1") != "0"
        self._monitor_now = False
        self.moments = self.moments_col = self.moments_ws = None      # collapse monitor (forward(monitor=True)): made on first use
        self.tail = None

    def _bind_params(self) -> None:
        super()._bind_params()
        self.tea_layers = [_layer_ptrs(self.flat, f"teacher_encoder.layers.{i}.", True) for i in range(self.cfg.l_enc)]

    def _fwd_stacks(self):
        enc, dec = super()._fwd_stacks()
        return [enc, (self.tea_layers, self.cfg.d_enc), dec]

    def _split_wgrad_shapes(self):
        c = self.cfg
        return [(c.d_enc, c.d_dec), (c.d_dec, c.d_enc)] + super()._split_wgrad_shapes()     # the two mappers between the stacks

    # ------------------------------------------------------------------------------------------------ arena
    def alloc(self, N: int, train: bool = True, G: int = 0, need_enc: int = 0, need_dec: int = 0) -> None:
        """The base's arena for N clips and, for training, G target groups per clip: the predictor runs N * G sequences."""
        super().alloc(N, train, seqs=dict(dec=N * (G or self.G or 1)), need_enc=need_enc, need_dec=need_dec)

    def _arena(self, N: int, train: bool) -> None:
        c, bf, f32, dev = self.cfg, torch.bfloat16, torch.float32, self.dev
        G = self.G = self.seqs["dec"] // N
        M, T, self.Mp = self.M, self.T, N * G * self.T
        Me, Md = self.cap_enc, self.cap_dec                   # rows of the student / predictor buffers (<= M / Mp)
        super()._arena(N, train)
        self._alloc_a8("tea", M, c.d_enc)                     # (the teacher runs beside the student: a scratch of its own)
        if not train:
            return
        if Md > 0:
            self._alloc_a8("dec", Md, c.d_dec)
        self.ctx_in = _empty(Me, c.d_enc, dtype=bf, device=dev)      # gathered context rows (<= Me)
        self.enc_in = _empty(Me, c.d_enc, dtype=f32, device=dev)     # ragged: local features of the context rows
        self.enc_in_b = _empty(Me, c.d_enc, dtype=bf, device=dev)
        self.tail_o = _empty(Md, c.d_dec, dtype=bf, device=dev)      # last predictor layer: target rows of o / x_in / do
        self.tail_x = _empty(Md, c.d_dec, dtype=f32, device=dev)
        self.tail_do = _empty(Md, c.d_dec, dtype=bf, device=dev)
        self.cf = _empty(Me, c.d_dec, dtype=bf, device=dev)          # contextual_features
        self.dec_in = _empty(Md, c.d_dec, dtype=f32, device=dev)
        self.dec_in_b = _empty(Md, c.d_dec, dtype=bf, device=dev)
        self.dec_out_b = _empty(Md, c.d_dec, dtype=bf, device=dev)
        self.dec_fm = _empty(Md, dtype=f32, device=dev)
        self.dec_fr = _empty(Md, dtype=f32, device=dev)
        self.preds = _empty(Md, c.d_enc, dtype=bf, device=dev)
        self.targets = _empty(M, c.d_enc, dtype=f32, device=dev)
        # teacher: outputs of the last top_k layers (fp32) and their per-clip (sum, sum of squares)
        nkeep = min(c.top_k, c.l_enc) if 1 < c.top_k <= 8 else 0
        self.tea_keep = [_empty(M, c.d_enc, dtype=f32, device=dev) for _ in range(nkeep)]
        self.tea_stats = _empty(max(nkeep, 1), N, ops.GROUP_STATS_SPLIT, 2, dtype=f32, device=dev)   # written by layernorm_fwd
        self.loss = torch.zeros(2, dtype=f32, device=dev)
        self.mse_ws = _empty(ops.workspace_bytes("wj_masked_mse", B=N, G=G, T=T) // 4, dtype=f32, device=dev)
        self.dpreds = _empty(Md, c.d_enc, dtype=bf, device=dev)
        self.d_cf = _empty(Me, c.d_dec, dtype=bf, device=dev)
        self.d_ctx_in = _empty(Me, c.d_enc, dtype=bf, device=dev)

    # ------------------------------------------------------------------------------------------------ forward
    def forward(self, audio: torch.Tensor, plan: MaskPlan, train: bool = True, drop_call: Optional[int] = None, monitor: bool = False,
                kept: Optional[Dict[str, Sequence[int]]] = None) -> None:
        """Training forward.  Results: self.loss[0], self.preds, self.targets, self.cf[:n_ctx], self.lf.
        train (module.training): with it, a stack whose EngineConfig rate is > 0 runs under dropout, its masks drawn from
        (self.drop_seed, drop_call); the backward of this forward uses the same.  Without it, or with both rates 0, the launches are
        exactly those of an engine without dropout.
        kept (LayerDrop, with `train` only): stack -> the sorted distinct indices of its layers that run in this forward and its
        backward; every other layer of the stack issues no launch, the stream passes it unchanged and its gradients stay the zeros of
        the cleared gradient buffer.  A stack that is not named runs every layer; the teacher always does.  An empty list is legal:
        the stack is then its final norm over its input.
        monitor: one wj_masked_moments right behind the loss, over the rows the loss uses; self.moments = (pred_var, target_var, n, 0)
        and self.moments_col (per-column mean and M2, what a data-parallel run merges).  Without it no launch, allocation or pointer
        of the step differs: the monitor's buffers are made by the first forward that asks for it."""
        N = audio.shape[0]
        self._monitor_now = bool(monitor)
        self._drop_now = {}
        if train and (self.cfg.dropout_enc > 0 or self.cfg.dropout_dec > 0):
            self._check_fp8()
            self._drop_now = {k: float(p) for k, p in (("enc", self.cfg.dropout_enc), ("dec", self.cfg.dropout_dec)) if p > 0}
            if drop_call is not None:
                self.drop_call = int(drop_call)
        self._kept_now = {}
        if train and kept:
            if self.fp8:
                self._check_fp8()        # (names the rates; an explicit kept list on an engine whose rates are 0 is refused below)
                raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with layerdrop (a kept list was handed to the forward)")
            for s, idx in kept.items():
                n, idx = len(self._stack(s)[0]), [int(i) for i in idx]
                if any(i < 0 or i >= n for i in idx) or any(b <= a for a, b in zip(idx, idx[1:])):
                    raise ValueError(f"kept[{s!r}] = {idx}: sorted distinct indices of the stack's {n} layers")
                self._kept_now[s] = idx
        if plan.N != N or plan.T != self.T or plan.G < 1:
            raise ValueError(f"mask plan is for {plan.N} clips x {plan.G} groups x {plan.T} tokens; the batch has {N} clips of {self.T} tokens")
        rag = self.ragged and plan.ragged_ok
        self.alloc(N, train=True, G=plan.G, need_enc=plan.n_ctx if rag else 0, need_dec=plan.n_dec if rag else 0)
        self.plan = plan
        self.audio = audio
        self._lean_now = self.use_side
        try:
            self._forward_body(audio, plan)
        finally:
            self._lean_now = False

    def _forward_body(self, audio: torch.Tensor, plan: MaskPlan) -> None:
        c, f = self.cfg, self.flat
        N = audio.shape[0]
        M, Mp, T, G = self.M, self.Mp, self.T, self.G
        De, Dd = c.d_enc, c.d_dec
        rag = self.ragged_step = self.ragged and plan.ragged_ok
        self._frontend(audio)
        # EMA teacher on the same local features (no mask, no final norm), joint instance-norm, mean of the last k layers:
        # independent of the student / predictor chain below, so it runs beside it on the side stream
        self.set_wt_need(plan.n_ctx if rag else M, plan.n_dec if rag else Mp)

        def beside():
            self._teacher_targets()
            if torch.is_grad_enabled():
                self.refresh_wt()       # W^T shadows for the backward's row-form dgrads: off the forward's critical path
        self._on_side(beside)
        self.wait_optimizer()           # (an update overlapped with this step's front-end: the transformer stacks' parameters)
        if rag and self.sparse_conv and torch.is_grad_enabled():
            # host-side list building + upload, hidden behind the forward kernels already queued.  (Building the lists later, behind
            # the student / predictor launches, measured the same outside the profiler -- 48.89 against 48.79 ms over three runs each --
            # and opened a 2-ms gap under rocprofv3, whose per-launch overhead makes the host the slower side.)
            self.front.active_rows(plan)
        n_ctx = plan.n_ctx
        final = dict(mean=self.enc_fm, rstd=self.enc_fr)
        if rag:
            # student encoder on the context rows only, packed per clip (non-context rows are dropped at jepa.py:399 and,
            # being key-masked, never influence a context row)
            ops.mask_gather_rows(self.lf, plan.keep, self.enc_in, n_rows=n_ctx, D=De, elem_bytes=4)
            if not c.norm_first_enc:        # (a pre-norm stack's first norm1 makes the bf16 GEMM operand itself)
                ops.mask_gather_rows(self.lf_b, plan.keep, self.enc_in_b, n_rows=n_ctx, D=De, elem_bytes=2)
            self._stack_fwd("enc", self.enc_in, self.enc_in_b, n_ctx, N, None, (plan.enc_off, max(plan.max_enc, 1)), acts=self._acts("enc"),
                            lean=True, y_bf16=self.ctx_in, **final)
        else:
            # student encoder over every token (keys restricted to the context), then the boolean-mask gather
            self._stack_fwd("enc", self.lf, self.lf_b, M, N, plan.ctx_u8, acts=self._acts("enc"),
                            y_f32=None if c.norm_first_enc else self.enc_out, y_bf16=self.enc_out_b, **final)
            ops.mask_gather_rows(self.enc_out_b, plan.keep, self.ctx_in, n_rows=n_ctx, D=De, elem_bytes=2)
        ops.gemm(self.ctx_in, f.ptr16("encoder_to_decoder_mapper.weight"), self.cf, M=n_ctx, N=Dd, K=De, lda=De, ldb=De, ldc=Dd,
                 bias=f.ptr32("encoder_to_decoder_mapper.bias"))
        # predictor over (context U group targets), one sequence per (clip, group)
        if rag:
            Md, dseq = plan.n_dec, (plan.dec_off, max(plan.max_dec, 1))
            ops.mask_scatter_fill_pos(self.cf, plan.inv, f.ptr32("mask_token"), self.pos_dec, B=N, T=T, D=Dd, G=G,
                                      out_f32=self.dec_in, out_bf16=self.dec_in_b, rows=plan.dec_rows, n_rows=Md)
        else:
            Md, dseq = Mp, None
            ops.mask_scatter_fill_pos(self.cf, plan.inv, f.ptr32("mask_token"), self.pos_dec, B=N, T=T, D=Dd, G=G,
                                      out_f32=self.dec_in, out_bf16=self.dec_in_b)
        self.tail = (plan.tgt_rows, plan.tgt_inv, plan.n_tgt) if (rag and self.trim_tail and plan.n_tgt > 0) else None
        Mo = plan.n_tgt if self.tail is not None else Md      # rows that leave the predictor
        self._stack_fwd("dec", self.dec_in, self.dec_in_b, Md, N * G, plan.vis_u8, dseq, acts=self._acts("dec"), sub=self.tail, lean=True,
                        y_bf16=self.dec_out_b, mean=self.dec_fm, rstd=self.dec_fr)
        ops.gemm(self.dec_out_b, f.ptr16("decoder_to_encoder_mapper.weight"), self.preds, M=Mo, N=De, K=Dd, lda=Dd, ldb=Dd,
                 ldc=De, bias=f.ptr32("decoder_to_encoder_mapper.bias"))
        self._join_side()               # teacher targets (side stream) are needed by the loss
        self._mse(None, None)
        if self._monitor_now:
            self._moments()

    def _loss_rows(self) -> dict:
        """The row list of self.preds for the loss and the monitor: the target rows (trimmed tail), the visible rows (ragged), none (dense)."""
        plan = self.plan
        if self.ragged_step and self.tail is not None:
            return dict(rows=plan.tgt_dense, n_rows=plan.n_tgt)          # preds hold the target rows only
        return dict(rows=plan.dec_rows, n_rows=plan.n_dec) if self.ragged_step else {}

    def _moments(self) -> None:
        """Collapse monitor: reads self.preds / self.targets only, behind the loss on the same stream, no host synchronisation."""
        N, G, T, De = self.N, self.G, self.T, self.cfg.d_enc
        need = ops.workspace_bytes("wj_masked_moments", B=N, G=G, T=T, D=De) // 8
        if self.moments is None or self.moments_col.shape[-1] != De:
            self.moments = torch.zeros(4, dtype=torch.float32, device=self.dev)
            self.moments_col = torch.zeros(2, 2, De, dtype=torch.float64, device=self.dev)
        if self.moments_ws is None or self.moments_ws.numel() < need:
            self.moments_ws = torch.empty(max(need, 1), dtype=torch.float64, device=self.dev)
        ops.masked_moments(self.preds, self.targets, self.plan.tgt_u8, self.moments, self.moments_ws, B=N, G=G, T=T, D=De,
                           col=self.moments_col, **self._loss_rows())

    def _mse(self, dpreds, gscale_ptr) -> None:
        c, plan = self.cfg, self.plan
        rows = self._loss_rows()
        if c.loss_kind == "mse":
            ops.masked_mse(self.preds, self.targets, plan.tgt_u8, self.loss, self.mse_ws, B=self.N, G=self.G, T=self.T, D=c.d_enc,
                           dpreds=dpreds, gscale_ptr=gscale_ptr, **rows)
        else:
            ops.masked_loss(self.preds, self.targets, plan.tgt_u8, self.loss, self.mse_ws, B=self.N, G=self.G, T=self.T, D=c.d_enc,
                            kind=c.loss_kind, beta=c.loss_beta, dpreds=dpreds, gscale_ptr=gscale_ptr, **rows)

    def dense_preds(self) -> torch.Tensor:
        """Predictions as the reference shapes them, bf16 [N*G, T, d_enc].  On a ragged step only the visible rows were
        computed (with the trimmed last layer: only the target rows); the others (zero loss weight on the reference,
        jepa.py:356) read 0."""
        N, G, T, De = self.N, self.G, self.T, self.cfg.d_enc
        if not self.ragged_step:
            return self.preds.view(N * G, T, De)
        out = _empty(N * G * T, De, dtype=torch.bfloat16, device=self.dev)
        if self.tail is not None:        # preds hold the target rows only: dense position -> packed row -> target row
            inv = torch.full((N * G * T,), -1, dtype=torch.int32, device=self.dev)
            inv[self.plan.tgt_dense.long()] = torch.arange(self.plan.n_tgt, dtype=torch.int32, device=self.dev)
        else:
            inv = self.plan.dec_map
        ops.unmask_rows_f32(self.preds, inv, out, M=N * G * T, D=De, src_is_f32=False, dst_is_bf16=True)
        return out.view(N * G, T, De)

    def _teacher_targets_pre(self) -> None:
        """Pre-norm teacher.  A layer's output is the stream s = x + branch, which exists only once the NEXT norm1 has added the
        branch (the last layer's: a plain add, the teacher has no final norm): that kernel writes a kept output to its own buffer,
        with the per-clip sums over s that wj_instnorm_mean needs."""
        c, N, M, De = self.cfg, self.N, self.M, self.cfg.d_enc
        a = self.scratch
        x, r = self.lf, None
        fused = 1 < c.top_k <= 8
        kept, nl = 0, len(self.tea_layers)
        for i in range(nl + 1):                    # step i materialises layer i - 1's output (i = nl: the stack's)
            keep = i > 0 and c.l_enc - (i - 1) <= c.top_k
            dest = self.tea_keep[kept] if (keep and fused) else None
            stats = self.tea_stats[kept] if dest is not None else None
            if i < nl:
                x_in = x
                x, r = self._layer_fwd_pre(self.tea_layers[i], a, x, r, M, De, c.h_enc, N, None, save=False, s_out=dest, s_stats=stats,
                                           stack="tea")
                s = dest if dest is not None else (x_in if i == 0 else a.x1)
            else:
                w = self.tea_layers[-1]            # (gamma / beta are not read: no normalised output is asked for)
                s = dest if dest is not None else (self.targets if c.top_k <= 1 else a.x1)
                ops.layernorm_pre_fwd(x, w.g1, w.be1, M=M, D=De, eps=c.ln_eps, r=r, s_f32=s, group_stats=stats,
                                      group_rows=self.T if stats is not None else 0)
            if keep and not fused and c.top_k > 1:   # mean over the layers actually kept: min(top_k, layers) (reference jepa.py:249-252)
                ops.instnorm_accumulate(s, self.targets, B=N, TD=self.T * De, accumulate=kept > 0, scale=1.0 / min(c.top_k, c.l_enc))
            kept += int(keep)
        if fused:
            ops.instnorm_mean(self.tea_keep[:kept], self.tea_stats, self.targets, B=N, TD=self.T * De)

    def _teacher_targets(self) -> None:
        if self.cfg.norm_first_enc:
            self._teacher_targets_pre()
            return
        c, N, M, De = self.cfg, self.N, self.M, self.cfg.d_enc
        a = self.scratch
        x, xb = self.lf, self.lf_b
        fused = 1 < c.top_k <= 8
        kept = 0
        xq = False
        for i, w in enumerate(self.tea_layers):
            keep = c.l_enc - i <= c.top_k
            if keep and fused:
                xq = self._layer_fwd(w, a, x, xb, M, De, c.h_enc, N, None, save=False, x2_out=self.tea_keep[kept],
                                     x2_stats=self.tea_stats[kept], stack="tea", xq_ready=xq)
                x, xb = self.tea_keep[kept], a.x2b
            else:
                xq = self._layer_fwd(w, a, x, xb, M, De, c.h_enc, N, None, save=False, stack="tea", xq_ready=xq)
                # ping-pong: the next layer reads x2/x2b while writing x1.. of the same scratch set, then x2 again;
                # x2 is only overwritten by the LAST kernel of the layer, after its readers have run (stream order).
                x, xb = a.x2, a.x2b
                if keep and c.top_k > 1:   # mean over the layers actually kept: min(top_k, layers) (reference jepa.py:249-252)
                    ops.instnorm_accumulate(x, self.targets, B=N, TD=self.T * De, accumulate=kept > 0, scale=1.0 / min(c.top_k, c.l_enc))
            kept += int(keep)
        if fused:
            ops.instnorm_mean(self.tea_keep[:kept], self.tea_stats, self.targets, B=N, TD=self.T * De)
        elif c.top_k <= 1:
            self.targets.copy_(x)

    # ------------------------------------------------------------------------------------------------ backward
    def backward(self, gscale_ptr: int = 0, on_grads_ready=None, accumulate: bool = False) -> None:
        """Gradients of self.loss[0] w.r.t. every trainable parameter -> flat.g32 (overwritten; accumulate=True: added to what the
        buffer holds -- every parameter-gradient output of this backward adds into it, so the one difference is the clear below).

        `on_grads_ready(tag)` is called (host side, stream-ordered) as sections of the flat gradient buffer become
        final: "dec" (predictor + both mappers), "enc:<i>" after encoder layer i, "front" at the end -- the hook the
        data-parallel wrapper uses to launch bucketed RCCL all-reduces that overlap the rest of the backward."""
        # partial training (freeze.py): the parameter-gradient work of a skipped unit is not launched, and the backward ends at the
        # floor, the lowest unit that is trainable and ran.  Nothing frozen: every test below passes, the launches are the parent's.
        c, f, plan = self.cfg, self.flat, self.plan
        fz = BackwardPlan(self._skip, c.l_enc, c.l_dec, self._kept_now)
        if on_grads_ready is None:
            ready = lambda tag: None
        elif self.use_side:
            # a section is final once BOTH streams are past this point: issue the hook (the bucket's all-reduce) from the
            # side stream after it has waited for the main stream, so that the main dgrad chain never stalls on it
            ready = lambda tag: self._on_side(lambda: (self._clear_frozen(tag), on_grads_ready(tag)))
        else:
            ready = lambda tag: (self._clear_frozen(tag), on_grads_ready(tag))
        section_final = ready

        def ready(tag):                  # a section is final only once the pending parameter-gradient folds have been queued
            if on_grads_ready is not None:       # (no consumer of sections: the folds go out in full groups and at the end)
                self._flush_folds()
            section_final(tag)
        enc_ready = set()

        def rest_ready():
            # the student layers nobody has reported yet (LayerDrop: those below the lowest one that ran; partial training: those
            # below the floor): final from the start, reported in descending order so that the listener hears every index once
            for j in range(c.l_enc - 1, -1, -1):
                if j not in enc_ready:
                    enc_ready.add(j)
                    ready(f"enc:{j}")
        if fz.floor is None:
            # everything is frozen: no launch.  The sections are reported all the same (the collectives of a data-parallel step are
            # the same on every rank and every step); the buffer reads zero, as behind any backward's clear
            self._folds = []             # (what _backward_open resets: entries an earlier backward that raised may have left)
            self._accum_open = bool(accumulate)
            if not accumulate and not f.g_clean:
                f.g32.zero_()
                f.g_clean = True
            if on_grads_ready is not None:
                ready("dec")
                rest_ready()
                on_grads_ready("front")
            return
        N, M, Mp, T, G = self.N, self.M, self.Mp, self.T, self.G
        De, Dd = c.d_enc, c.d_dec
        self._backward_open(accumulate)
        rag = self.ragged_step
        Md, dseq = (plan.n_dec, (plan.dec_off, max(plan.max_dec, 1))) if rag else (Mp, None)
        Me, eseq = (plan.n_ctx, (plan.enc_off, max(plan.max_enc, 1))) if rag else (M, None)
        self._mse(self.dpreds, gscale_ptr if gscale_ptr else None)
        bw = self.bw["dec"]
        # decoder_to_encoder_mapper
        Mo = plan.n_tgt if (rag and self.tail is not None) else Md       # rows that left the predictor
        if not fz.skipped("decoder_to_encoder_mapper"):
            self._colsum_bf16(self.dpreds, f.gptr("decoder_to_encoder_mapper.bias"), M=Mo, N=De, ldx=De)
            self._wgrad(self.dpreds, self.dec_out_b, f.gptr("decoder_to_encoder_mapper.weight"), De, Dd, Mo)
        dy = None
        if fz.below("decoder_to_encoder_mapper"):
            ops.gemm(self.dpreds, f.ptr16("decoder_to_encoder_mapper.weight"), bw["dx1"], M=Mo, N=Dd, K=De, lda=De, ldb=Dd, ldc=Dd,
                     b_trans=1, epilogue=ops.EPI_ADD_F32)
            run, stop = fz.stack_walk("decoder", self._kept("dec"))
            walk = {} if (run and stop is None) else dict(layers_run=run, stop=stop)
            if run or not fz.skipped("decoder.norm"):
                dy = self._stack_bwd("dec", self.dec_in, self.dec_in_b, Md, N * G, plan.vis_u8, dseq, sub=self.tail if rag else None, **walk)
        n_ctx = plan.n_ctx
        if fz.reaches("mask_token"):
            # the mask-token gradient leaves the kernel as one partial row per workgroup, folded with the other deferred folds (round 4:
            # 384 global float atomics per workgroup into the same 384 addresses); deterministic mode: never the kernel's own atomics
            if fz.skipped("mask_token"):         # (the data gradient only)
                ops.mask_scatter_fill_pos_bwd(dy, plan.inv, self.d_cf, None, B=N, T=T, D=Dd, G=G, rowmap=plan.dec_map if rag else None)
            else:
                sf_rows = ops.scatter_fill_bwd_partial_rows(N, T)
                form, ws = self._fold_form(Dd, True, fits=sf_rows * Dd * 4 <= self._red_bytes)
                if form == "now" and sf_rows * Dd * 4 > self.red_ws.numel() * 4:
                    raise RuntimeError("deterministic mode: the mask-token partial rows do not fit the reduction scratch")
                ops.mask_scatter_fill_pos_bwd(dy, plan.inv, self.d_cf, f.gptr("mask_token"), B=N, T=T, D=Dd, G=G,
                                              rowmap=plan.dec_map if rag else None, partials=ws)
                self._fold(form, ws, Dd, sf_rows, f.gptr("mask_token"), None, None, Dd)
        if fz.reaches("encoder_to_decoder_mapper"):
            # encoder_to_decoder_mapper (rows = gathered context tokens)
            if not fz.skipped("encoder_to_decoder_mapper"):
                self._colsum_bf16(self.d_cf, f.gptr("encoder_to_decoder_mapper.bias"), M=n_ctx, N=Dd, ldx=Dd)
                self._wgrad(self.d_cf, self.ctx_in, f.gptr("encoder_to_decoder_mapper.weight"), Dd, De, n_ctx)
            if fz.below("encoder_to_decoder_mapper"):
                ops.gemm(self.d_cf, f.ptr16("encoder_to_decoder_mapper.weight"), self.d_ctx_in, M=n_ctx, N=De, K=Dd, lda=Dd, ldb=De,
                         ldc=De, b_trans=1)
        ready("dec")
        if fz.below("encoder_to_decoder_mapper"):
            bw = self.bw["enc"]
            if rag:
                ops.unmask_rows_f32(self.d_ctx_in, None, bw["dx1"], M=Me, D=De)      # packed rows: a widening copy
            else:
                ops.unmask_rows_f32(self.d_ctx_in, plan.inv, bw["dx1"], M=M, D=De)
            every = "enc" not in self._kept_now              # no LayerDrop in this step: every layer ran

            def flushed(i):
                # the weight gradients of two layers share a grouped launch: a layer's section of the gradient buffer is final (and its
                # all-reduce bucket may go) once the launch that carries it has been queued.  LayerDrop: the section of a layer that did
                # not run is final from the start (the zeros of the cleared buffer, or what earlier micro-batches left); it is reported
                # with the next layer below it that ran, so the listener still hears every index once, in descending order.
                for j in range(min(c.l_enc - 1, i + bw["group"] - 1) if every else c.l_enc - 1, i - 1, -1):
                    if j not in enc_ready:
                        enc_ready.add(j)
                        ready(f"enc:{j}")
            first = (self.enc_in, self.enc_in_b) if rag else (self.lf, self.lf_b)
            run, stop = fz.stack_walk("encoder", self._kept("enc"))
            walk = {} if (run and stop is None) else dict(layers_run=run, stop=stop)
            dy = self._stack_bwd("enc", first[0], first[1], Me, N, plan.ctx_u8, eseq, flushed=flushed, **walk)
        if len(enc_ready) < c.l_enc:
            rest_ready()                                 # layers below the lowest one that ran (or all of them: none ran)
        if fz.reaches("front"):
            self._frontend_bwd(dy, rag, plan)
        self._backward_close()
        if on_grads_ready is None:
            self._clear_frozen(None)
        else:
            self._clear_frozen("front")
            on_grads_ready("front")

    # ------------------------------------------------------------------------------------------------ EMA
    def ema_step(self, r: float) -> None:
        f = self.flat
        self.wait_optimizer()
        ops.ema_update(f.p32.data_ptr() + 4 * f.enc_offset, f.t32, f.enc_numel, r, teacher_bf16=f.t16)
