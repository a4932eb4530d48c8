"""The conv front-end: everything between the bf16 audio and post[-1], the last conv layer's output, forward and backward.

Layout: channels-last [clip][row][C] with per-clip row counts P_l chosen so that P_{l-1} = stride_l * P_l; a strided conv is then ONE
GEMM with lda = stride*C and K = k*C over all clips (rows >= L_l of a clip are padding, kept at zero).  Every audio channel of a
ConvChannelFeatureExtractor is a mono clip of one channel-major batch (conv clip c*N + n), through its own or the shared stack.

One ConvFrontend serves the training / inference engine (parameters from FlatParams) and the stand-alone extractor forward
(standalone.py, parameters from the nn.Module): the norm mode enters the forward at two points, the layer-0 entry and the form of a
later layer (one EPI_CONV_GELU GEMM, or an EPI_BF16 GEMM (+ bias) and a LayerNorm + GELU pass).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .upload import pack_upload


def _empty(*shape, dtype, device):
    """Arena buffers are uninitialised by design (every kernel writes what a later kernel reads).  WJ_ARENA_FILL=nan poisons
    them instead, so that a read of never-written memory shows up as NaN in the results (tools/debug_order.py)."""
    if os.environ.get("WJ_ARENA_FILL", "") == "nan":
        if not dtype.is_floating_point:          # fp8 operand bytes: 0x7f is the e4m3 NaN encoding
            return torch.full(shape, 0x7f, dtype=dtype, device=device)
        return torch.full(shape, float("nan"), dtype=dtype, device=device)
    return torch.empty(*shape, dtype=dtype, device=device)


def padded_rows(nrows: int, width: int, dtype, device, lead: int = 2, tail: int = 8) -> Tuple[torch.Tensor, int]:
    """A zero-initialised [lead + nrows + tail][width] buffer; returns (tensor, pointer to row 0).  The dgrad GEMMs of the backward
    read from up to U - 1 rows before row 0 of d(pre[l]) and prefetch past the last row: both land in these zero rows."""
    t = torch.zeros((lead + nrows + tail) * width, dtype=dtype, device=device)
    return t, t.data_ptr() + lead * width * t.element_size()


def conv_geometry(n_samples: int, spec) -> Tuple[List[int], List[int]]:
    """Valid output lengths L_l and padded per-clip row counts P_l with P_{l-1} = stride_l * P_l and enough zero
    padding rows for the dgrad taps (P_l - L_l >= ceil(k_l / s_l) - 1, at least 1)."""
    L, cur = [], n_samples
    for _, k, s in spec:
        cur = (cur - k) // s + 1
        L.append(cur)
    n = len(spec)
    need = [max(1, -(-spec[l][1] // spec[l][2]) - 1) for l in range(n)]
    p_last = L[-1] + need[-1]
    while True:
        P = [0] * n
        P[-1] = p_last
        for l in range(n - 2, -1, -1):
            P[l] = P[l + 1] * spec[l + 1][2]
        if all(P[l] >= L[l] + need[l] for l in range(n)):
            return L, P
        p_last += 1


def conv_active_rows(keep: np.ndarray, P: Sequence[int], spec) -> Dict[int, Tuple[np.ndarray, np.ndarray]]:
    """Rows of every conv layer's output that can carry a gradient when only `keep` [N, T] (bool) rows of the LAST layer's
    output do (the student sees the context tokens only, so ~80 % of the conv backward would multiply zeros).

    Returns {l: (act, ext)} of int32 GLOBAL row indices (clip * P[l] + row), ascending:
      act[l]: rows of layer l's output gradient that are written this step (consumed by GELU', wgrad, and cleared after);
      ext[l]: act[l] grown by the dgrad halo (ceil(k/s) - 1 rows after every run): the logical rows of the dgrad GEMM, whose
              outputs s*g + rho, rho < s, are exactly act[l-1].
    Layer 0 (no GEMM dgrad below it): (act, per-clip offsets int32 [N+1] into act)."""
    N, T = keep.shape
    edge = np.diff(np.concatenate([np.zeros((N, 1), np.int8), keep.astype(np.int8), np.zeros((N, 1), np.int8)], axis=1), axis=1)
    clip, start = np.nonzero(edge == 1)
    _, end = np.nonzero(edge == -1)          # same (clip, position) order: the i-th end closes the i-th start

    def expand(clip, start, end, rows_per_clip):
        n = end - start
        if n.size == 0:
            return np.zeros(0, np.int32)
        first = np.cumsum(n) - n
        return (np.repeat(clip.astype(np.int64) * rows_per_clip + start - first, n) + np.arange(int(n.sum()))).astype(np.int32)

    out: Dict[int, Tuple[np.ndarray, Optional[np.ndarray]]] = {}
    for l in range(len(spec) - 1, 0, -1):
        _, k, s = spec[l]
        act = expand(clip, start, end, P[l])
        grown = end + (-(-k // s) - 1)
        if start.size:                       # merge runs that now touch or overlap inside a clip
            new = np.ones(start.size, bool)
            new[1:] = (clip[1:] != clip[:-1]) | (start[1:] > grown[:-1])
            head = np.flatnonzero(new)
            clip, start, grown = clip[head], start[head], np.maximum.reduceat(grown, head)
        out[l] = (act, expand(clip, start, grown, P[l]))
        start, end = start * s, grown * s
    per_clip = np.bincount(clip, weights=end - start, minlength=N).astype(np.int64)
    out[0] = (expand(clip, start, end, P[0]), np.concatenate([[0], np.cumsum(per_clip)]).astype(np.int32))
    return out


class ConvLayerParams:
    """Parameters of one (stack, layer): device pointers or tensors.  Layer 0: w bf16 [C][C_in][k]; layers 1..: w the fp32 master
    [C][C][k] (the GEMM layouts are made from it).  b: conv bias f32 or None.  gamma / beta: the layer's norm (GroupNorm on layer 0 of
    the default mode, LayerNorm on every layer of mode "layer_norm"; None where the layer has none).  g*: where the gradients go
    (None: forward only).  eps: None leaves the kernels' default."""
    __slots__ = ("w", "b", "gamma", "beta", "gw", "gb", "ggamma", "gbeta", "eps")

    def __init__(self, w, b=None, gamma=None, beta=None, gw=None, gb=None, ggamma=None, gbeta=None, eps: Optional[float] = None):
        self.w, self.b, self.gamma, self.beta = w, b, gamma, beta
        self.gw, self.gb, self.ggamma, self.gbeta = gw, gb, ggamma, gbeta
        self.eps = {} if eps is None else {"eps": eps}


class ConvFrontend:
    def __init__(self, spec, in_channels: int, n_samples: int, streams: int, params: Sequence[Sequence[ConvLayerParams]], ln: bool, device,
                 backward: bool = True):
        """params[stack][layer]: one stack (every stream shares it) or one per stream; in_channels: per stream.  ln: mode "layer_norm".
        backward=False keeps no dgrad layouts and no weight-gradient scratch (a forward-only front-end)."""
        self.spec, self.C_in, self.n_samples, self.S = [tuple(x) for x in spec], in_channels, n_samples, streams
        self.params, self.ln, self.dev = params, ln, device
        assert len(params) in (1, streams)
        self.C = self.spec[-1][0]
        self.L, self.P = conv_geometry(n_samples, self.spec)
        self.nl = len(self.spec)
        # per layer l >= 1: the phases rho of its stride with their tap counts U (a phase with no tap, k < s, writes nothing)
        self.phases = [None] + [[(rho, len(range(rho, k, s))) for rho in range(s) if len(range(rho, k, s)) > 0] for _, k, s in self.spec[1:]]
        self.empty_phase = [False] + [len(self.phases[l]) < self.spec[l][2] for l in range(1, self.nl)]
        # per (stack, layer >= 1): the forward GEMM layout, one dgrad layout per phase, the fp32 weight-gradient scratch
        C, bf = self.C, torch.bfloat16
        self.wp, self.wd, self.dwp = ([[None] * self.nl for _ in params] for _ in range(3))
        for si in range(len(params)):
            for l in range(1, self.nl):
                k = self.spec[l][1]
                self.wp[si][l] = _empty(C, k * C, dtype=bf, device=device)
                if backward:
                    self.wd[si][l] = [_empty(U * C, C, dtype=bf, device=device) for _, U in self.phases[l]]
                    self.dwp[si][l] = torch.zeros(C, k * C, dtype=torch.float32, device=device)
        self.has_backward = backward
        self.w_fresh = False
        self.grads_dirty = False
        self.N = 0

    # ------------------------------------------------------------------------------------------------ arena
    def alloc(self, N: int, train: bool) -> None:
        """Activations (post-GELU, and pre-GELU for layers >= 1), norm statistics and, for training, their gradients, for N clips."""
        C, S, P, dev, bf, f32 = self.C, self.S, self.P, self.dev, torch.bfloat16, torch.float32
        self.N, self.train = N, train
        Nc = N * S                                    # mono conv clips (channel-major: clip index c*N + n)
        self.post, self.post_ptr, self.pre, self.pre_ptr = [], [], [None], [0]
        self.dpost, self.dpost_ptr, self.dpre, self.dpre_ptr = [], [], [None], [0]
        for l in range(self.nl):
            for on, ts, ps in ((True, self.post, self.post_ptr), (l > 0, self.pre, self.pre_ptr), (train, self.dpost, self.dpost_ptr),
                               (train and l > 0, self.dpre, self.dpre_ptr)):
                if on:
                    t, p = padded_rows(Nc * P[l], C, bf, dev)
                    ts.append(t); ps.append(p)
        _, k0, s0 = self.spec[0]
        taps = self.C_in * k0
        conv0_dims = dict(N=N, C_in=self.C_in, C=C, k=k0, L_out=self.L[0])      # per stream: N clips a call
        # the layer-0 argument block, shared by the four layer-0 entries: geometry + the distance between a stream's clips
        self.conv0_kw = dict(conv0_dims, L=self.n_samples, stride=s0, P=P[0], audio_clip_stride=S * self.C_in * self.n_samples if S > 1 else 0)
        if self.ln:
            # per-row LayerNorm statistics of every conv layer; layer 0's backward scratch (dense form: the largest)
            self.cl_mean = [_empty(Nc * P[l], dtype=f32, device=dev) for l in range(self.nl)]
            self.cl_rstd = [_empty(Nc * P[l], dtype=f32, device=dev) for l in range(self.nl)]
            self.cl_ws_b = _empty(ops.workspace_bytes("wj_conv0_ln_gelu_bwd", max_rows=0, **conv0_dims) // 4, dtype=f32, device=dev) if train else None
        else:
            self.gn_stats = _empty(2, Nc, C, dtype=f32, device=dev)
            self.gn_ws = _empty(ops.workspace_bytes("wj_conv0_gn_gelu_fwd", **conv0_dims) // 4, dtype=f32, device=dev)
            self.gn_ws_b = _empty(ops.workspace_bytes("wj_conv0_gn_gelu_bwd", max_rows=0, **conv0_dims) // 4, dtype=f32, device=dev) if train else None
            self.gn_yx = _empty(Nc, C, taps, dtype=f32, device=dev) if train else None     # forward sums the backward needs
            self.gn_x1 = _empty(Nc, taps, dtype=f32, device=dev) if train else None
        self.groups = self.stack_groups()

    def stack_groups(self):
        """[(stack index, first conv clip, clips)] for the conv GEMMs of a batch of self.N clips: one group over all S*N mono
        clips when the streams share their weights, one group of N clips per stream otherwise (clips are channel-major)."""
        if len(self.params) == 1:
            return [(0, 0, self.N * self.S)]
        return [(c, c * self.N, self.N) for c in range(self.S)]

    def layer0_args(self, audio: torch.Tensor, ch: int):
        """Stream ch of `audio` bf16 [N, S * C_in, L] for a layer-0 entry: (pointer to its first sample, geometry keywords), and the
        stream's parameters."""
        return audio.data_ptr() + ch * self.n_samples * 2, self.conv0_kw, self.params[min(ch, len(self.params) - 1)][0]

    def tokens(self) -> torch.Tensor:
        """post[-1] without its padding: bf16 [N, S * T, C], channel-major within a clip (a copy)."""
        N, S, C, P, T = self.N, self.S, self.C, self.P[-1], self.L[-1]
        x = self.post[-1][2 * C:(2 + N * S * P) * C].view(S, N, P, C)[:, :, :T]
        return x.permute(1, 0, 2, 3).reshape(N, S * T, C).contiguous()

    # ------------------------------------------------------------------------------------------------ forward
    def weight_layouts(self) -> None:
        """GEMM layouts of conv layers 1.. from the fp32 masters (20 launches of ~5 us).  Issued by the forward AFTER the conv0 kernels
        are queued: at the start of a step the GPU is idle, and the host needs ~15 us per launch -- behind conv0 (1.1 ms) they cost nothing,
        in front of it they were 0.3 ms of idle GPU per step (rocprofv3 trace, tools/trace_gaps.py)."""
        if self.w_fresh:
            return
        C = self.C
        for si, stack in enumerate(self.params):
            for l in range(1, self.nl):
                _, k, s = self.spec[l]
                ops.conv_weight_layout(stack[l].w, self.wp[si][l], C_out=C, C_in=C, k=k, mode=0)
                if self.has_backward:
                    for (rho, U), wd in zip(self.phases[l], self.wd[si][l]):
                        ops.conv_weight_layout(stack[l].w, wd, C_out=C, C_in=C, k=k, mode=1, stride=s, rho=rho, U=U)
        self.w_fresh = True

    def forward(self, audio: torch.Tensor) -> None:
        """audio bf16 [N, S * C_in, L] -> post[l], pre[l] and the norm statistics of every layer.
        mode "default": conv0 + GroupNorm + GELU, then one implicit GEMM with the fused GELU epilogue per layer.
        mode "layer_norm": the fused layer-0 kernel, then per layer the conv GEMM (bf16 pre-activations, + bias) and one LayerNorm + GELU
        pass over its rows -> post[l] (bf16, clip padding rows 0); per-row mean / rstd kept for the backward."""
        N, C, P, L = self.N, self.C, self.P, self.L
        grad = torch.is_grad_enabled() and self.train                  # (an inference arena keeps no backward sums)
        for ch in range(self.S):                          # every stream: N mono clips (ConvFeatureExtractor: one stream, C_in channels)
            audio_p, dims, p = self.layer0_args(audio, ch)
            c0 = ch * N                                   # first conv clip of this stream
            r0 = c0 * P[0]
            if self.ln:
                ops.conv0_ln_fwd(audio_p, p.w, p.b, p.gamma, p.beta, self.post_ptr[0] + r0 * C * 2, self.cl_mean[0][r0:], self.cl_rstd[0][r0:],
                                 **dims, **p.eps)
            else:
                ops.conv0_fwd(audio_p, p.w, p.gamma, p.beta, self.post_ptr[0] + r0 * C * 2, self.gn_stats[0, c0:], self.gn_stats[1, c0:],
                              self.gn_ws, yx=self.gn_yx[c0:] if grad else None, x1=self.gn_x1[c0:] if grad else None, **dims)
        self.weight_layouts()
        for l in range(1, self.nl):
            _, k, s = self.spec[l]
            for si, c0, nclips in self.groups:
                p, r0, rows = self.params[si][l], c0 * P[l], nclips * P[l]
                x, pre, post = self.post_ptr[l - 1] + c0 * P[l - 1] * C * 2, self.pre_ptr[l] + r0 * C * 2, self.post_ptr[l] + r0 * C * 2
                shape = dict(M=rows, N=C, K=k * C, lda=s * C, ldb=k * C, ldc=C)
                if self.ln:
                    ops.gemm(x, self.wp[si][l], pre, bias=p.b, epilogue=ops.EPI_BF16, **shape)
                    ops.conv_ln_gelu_fwd(pre, p.gamma, p.beta, post, M=rows, C=C, mean=self.cl_mean[l][r0:], rstd=self.cl_rstd[l][r0:],
                                         seg_rows=P[l], seg_valid=L[l], **p.eps)
                else:
                    ops.gemm(x, self.wp[si][l], pre, C2=post, epilogue=ops.EPI_CONV_GELU, seg_rows=P[l], seg_valid=L[l], **shape)

    # ------------------------------------------------------------------------------------------------ backward
    def backward(self, eng, audio: torch.Tensor, plan) -> None:
        """d(post[-1]) (in dpost[-1]) -> the conv stacks' parameter gradients.  plan: the mask plan of a ragged step whose backward
        visits the active rows only (active_rows), None: every row.  eng: the engine, for its fold forms (_fold_form / _fold, red_ws),
        its deterministic mode (_det_kw, deterministic), its side stream (_on_side / _join_side) and its conv switches."""
        sparse = plan is not None
        lists = None
        if sparse:
            lists = self.active_rows(plan)
            if self.grads_dirty:             # a dense step left gradients everywhere: restore the all-zero state once
                for t in self.dpost + self.dpre[1:]:
                    t.zero_()
                self.grads_dirty = False
        else:
            self.grads_dirty = True
        side_wgrad = sparse and eng.use_side and eng.conv_wgrad_side
        # mode="layer_norm": the LayerNorm sits between GELU' and the convolution, so GELU' cannot ride in the dgrad epilogue: plain dgrads
        # into d(post[l - 1]) and one wj_conv_ln_gelu_bwd per layer where the default mode runs wj_gelu_bwd_bf16
        fuse_gelu = sparse and eng.fuse_conv_gelu_bwd and not self.ln
        late_clear = []
        for l in range(self.nl - 1, 0, -1):
            if self.empty_phase[l]:
                self.dpost[l - 1].zero_()
            for gi in range(len(self.groups)):
                self._layer_bwd(eng, l, gi, lists[l][gi] if sparse else None, side_wgrad, fuse_gelu, late_clear)
        C = self.C
        for ch in range(self.S):             # layer 0: one call per stream (N mono clips each; ConvFeatureExtractor: one stream)
            audio_p, dims, p = self.layer0_args(audio, ch)
            c0 = ch * self.N
            r0 = c0 * self.P[0]
            dact = self.dpost_ptr[0] + r0 * C * 2
            listed = {}
            if sparse:
                rows0, n0, off0, max0 = lists[0][ch]
                listed = dict(rows=rows0, row_off=off0, max_rows=max0)
            if self.ln:
                ops.conv0_ln_bwd(audio_p, p.w, p.b, p.gamma, p.beta, self.cl_mean[0][r0:], self.cl_rstd[0][r0:], dact, p.gw, p.gb, p.ggamma,
                                 p.gbeta, self.cl_ws_b, **dims, **listed)
            else:
                ops.conv0_bwd(audio_p, p.w, p.gamma, p.beta, self.gn_stats[0, c0:], self.gn_stats[1, c0:], dact, p.gw, p.ggamma, p.gbeta,
                              self.gn_ws_b, yx=self.gn_yx[c0:], x1=self.gn_x1[c0:], **dims, **listed)
            if sparse:
                ops.zero_rows(dact, rows0, n_rows=n0, row_bytes=C * 2)
        if late_clear:
            eng._join_side()                 # the side stream's conv weight gradients have read d(pre[l]): clear the rows now
            for ptr, act, n_act in late_clear:
                ops.zero_rows(ptr, act, n_rows=n_act, row_bytes=C * 2)

    def _layer_bwd(self, eng, l: int, gi: int, listed, side_wgrad: bool, fuse_gelu: bool, late_clear: list) -> None:
        """Layer l >= 1 of stack group gi: d(post[l]) -> d(pre[l]) (GELU', and the LayerNorm in mode "layer_norm"), the weight gradient,
        and one dgrad GEMM per phase into d(post[l - 1]).

        listed = (act, n_act, ext, n_ext), the sparse form: only act[l] rows of this layer's output gradient are non-zero.  Every
        gradient buffer is all-zero outside the rows written this step (they are cleared again at the end), so the dgrad taps may read
        neighbours freely.  The lists hold rows of the WHOLE buffer, a group takes its contiguous slice of them: base pointers are the
        buffers' and M their row count.  Dense (None): the group's own rows, by offset."""
        C, P, nl = self.C, self.P, self.nl
        _, k, s = self.spec[l]
        si, c0, nclips = self.groups[gi]
        p, dwp = self.params[si][l], self.dwp[si][l]
        if listed is not None:
            row0, M = 0, self.N * self.S * P[l]
            act, n_act, ext, n_ext = listed
            pick = dict(rows=act, n_rows=n_act, clear_dpost=l < nl - 1)
        else:
            row0, M = c0 * P[l], nclips * P[l]
            act, n_act, ext, n_ext = None, M, None, M
            pick = {}
        off, offp = row0 * C * 2, row0 * s * C * 2            # byte offsets of the first row (layers l, l-1: P[l-1] = s * P[l])
        dpost, pre, dpre = self.dpost_ptr[l] + off, self.pre_ptr[l] + off, self.dpre_ptr[l] + off
        if not side_wgrad:
            dwp.zero_()
        if self.ln:
            # its dgamma | dbeta | dbias partial rows take the fold forms of the engine's LayerNorm backward
            args = (dpost, pre, self.cl_mean[l][row0:], self.cl_rstd[l][row0:], p.gamma, p.beta, dpre)
            kw = dict(M=M, C=C, seg_rows=P[l], seg_valid=self.L[l], **pick)
            form, ws = eng._fold_form(3 * C, True)
            if form == "slot":
                ops.conv_ln_gelu_bwd(*args, ws, **kw)
                eng._fold(form, ws, 3 * C, ops.conv_ln_bwd_partial_rows(n_act, C), p.ggamma, p.gbeta, p.gb, C)
            else:                                # the entry folds its partial rows itself (in order when deterministic)
                ops.conv_ln_gelu_bwd(*args, eng.red_ws, dgamma=p.ggamma, dbeta=p.gbeta, dbias=p.gb, deterministic=eng.deterministic, **kw)
        elif not (fuse_gelu and l < nl - 1):
            # (layers below the top one: d(pre) was written by the dgrad of the layer above, GELU' fused in its epilogue)
            ops.gelu_bwd_bf16(dpost, pre, dpre, 0 if pick else M * C, row_elems=C if pick else 0, **pick)

        def wgrad():
            if side_wgrad:
                dwp.zero_()
            if n_act > 0:
                ops.gemm(dpre, self.post_ptr[l - 1] + offp, dwp, M=C, N=k * C, K=n_act, lda=C, ldb=s * C, ldc=k * C, a_trans=1, b_trans=1,
                         epilogue=ops.EPI_ATOMIC_F32, split_k=ops.pick_split_k(C, k * C, n_act), rowmap=act, **eng._det_kw())
            ops.conv_weight_layout(dwp, p.gw, C_out=C, C_in=C, k=k, mode=2)
        if not side_wgrad:
            wgrad()
        elif n_act > 0:
            # The layer's weight gradient (+ its scratch clear and the layout fold) on the SIDE stream: at this point of the
            # backward that stream is idle (every transformer weight gradient is out), and the main chain goes on with this
            # layer's dgrads, GELU' and the layer-0 pass -- d(pre[l]) is read by both and cleared only behind the join at the end.
            eng._on_side(wgrad)
        if n_ext > 0:
            # fused: the rows this GEMM writes (s g + rho, g in ext) are exactly act[l - 1]: d(pre[l - 1]) = bf16(d(post)) * gelu'(pre)
            # straight from its epilogue -- the bits a bf16 d(post) tensor + wj_gelu_bwd_bf16 over act[l - 1] would give
            fused = fuse_gelu and l - 1 >= 1
            out = (self.dpre_ptr if fused else self.dpost_ptr)[l - 1] + offp
            for (rho, U), wd in zip(self.phases[l], self.wd[si][l]):
                epi = dict(epilogue=ops.EPI_MUL_GELU_GRAD_Z, aux=self.pre_ptr[l - 1] + offp + rho * C * 2) if fused else {}
                ops.gemm(dpre - (U - 1) * C * 2, wd, out + rho * C * 2, M=n_ext, N=C, K=U * C, lda=C, ldb=C, ldc=s * C, b_trans=1,
                         rowmap=ext, **epi)
        if side_wgrad:
            late_clear.append((self.dpre_ptr[l], act, n_act))
        elif listed is not None:
            ops.zero_rows(self.dpre_ptr[l], act, n_rows=n_act, row_bytes=C * 2)

    def active_rows(self, plan):
        """Device copies of conv_active_rows for this plan (cached on the plan: mask sets are reused by the data source).
        {l >= 1: [per stack group (act, n_act, ext, n_ext)]} with rows of the WHOLE layer buffer (a group's rows are a contiguous
        slice of the ascending list: conv clips are channel-major), {0: [per stream (rows, n, row_off, max_rows)]} with rows
        relative to the stream's first clip (one conv0 call per stream)."""
        key = (self.N, self.S, len(self.params), tuple(self.P))
        cached = getattr(plan, "_conv_rows", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        N, S, Tc = self.N, self.S, self.L[-1]
        keep = (plan.ctx_u8.cpu().numpy() == 0) if plan.ctx_np is None else ~plan.ctx_np
        if S > 1:                            # tokens (n, c, t) -> conv clip c*N + n
            keep = np.ascontiguousarray(keep.reshape(N, S, Tc).transpose(1, 0, 2)).reshape(S * N, Tc)
        lists = conv_active_rows(keep, self.P, self.spec)
        pad = np.zeros(256, np.int32)        # the k-gather GEMM prefetches indices up to 256 entries past the end
        # every list of the step in ONE host -> device copy
        act0, off0 = lists[0]
        host, keys = [], []
        for l, (act, ext) in lists.items():
            if l == 0:
                continue
            host += [np.concatenate([act, pad]).astype(np.int32), np.concatenate([ext, pad]).astype(np.int32)]
            keys += [("act", l), ("ext", l)]
        per0_host = []
        for ch in range(S):
            lo, hi = int(off0[ch * N]), int(off0[(ch + 1) * N])
            rows = (act0[lo:hi] - ch * N * self.P[0]).astype(np.int32)
            off = (off0[ch * N:(ch + 1) * N + 1] - lo).astype(np.int32)
            per0_host.append((rows, off))
            host += [np.concatenate([rows, pad]).astype(np.int32), np.concatenate([off, pad]).astype(np.int32)]
            keys += [("rows0", ch), ("off0", ch)]
        dev = dict(zip(keys, pack_upload(host, self.dev)))

        out = {}
        for l, (act, ext) in lists.items():
            if l == 0:
                continue
            d_act, d_ext = dev[("act", l)], dev[("ext", l)]
            per = []
            for _, c0, nclips in self.groups:
                lo, hi = c0 * self.P[l], (c0 + nclips) * self.P[l]
                a0, a1 = np.searchsorted(act, [lo, hi])
                e0, e1 = np.searchsorted(ext, [lo, hi])
                per.append((d_act.data_ptr() + 4 * int(a0), int(a1 - a0), d_ext.data_ptr() + 4 * int(e0), int(e1 - e0)))
            out[l] = per
            out[("keep", l)] = (d_act, d_ext)        # owners of the pointers above
        per0 = []
        for ch, (rows, off) in enumerate(per0_host):
            per0.append((dev[("rows0", ch)], int(rows.size), dev[("off0", ch)], int(np.diff(off).max()) if off.size > 1 else 0))
        out[0] = per0
        plan._conv_rows = (key, out)
        return out
