"""The encoder base of the step engines: the conv front-end and trainable transformer stacks, forward and backward, on one MI355X.

The host side of the hot path: a fixed sequence of C-ABI kernel launches over a pre-allocated activation arena (no autograd graph,
no allocator traffic in the step, no host synchronisation).  Activations are token-major bf16/fp32 buffers sized once per batch
size; the residual stream is fp32 and every GEMM operand is bf16, exactly the dtype flow bf16 autocast produces on the reference.

EncoderEngine runs the front-end and the student stack ("enc") and knows no masks, predictor, teacher or loss: a step engine --
engine.JepaEngine, denoiser.DenoiserEngine -- adds those, and any further trainable stack, by extending BW_RING / MODULE.
The conv front-end (audio -> the last conv layer's output, and its backward) is conv_frontend.ConvFrontend; the engine adds
feature_norms, the mapper and the positions behind it (_frontend) and their backward in front of it (_frontend_bwd).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import ops
from .conv_frontend import ConvFrontend, ConvLayerParams, _empty
from .params import FlatParams


@dataclass
class EngineConfig:
    conv_spec: Sequence[Tuple[int, int, int]]
    in_channels: int
    n_samples: int          # waveform samples per clip (32159)
    d_enc: int
    h_enc: int
    l_enc: int
    d_dec: int = 0          # the predictor (JepaEngine); an encoder-only engine leaves the four out
    h_dec: int = 0
    l_dec: int = 0
    top_k: int = 1
    streams: int = 1        # audio channels run as separate MONO conv stacks (ConvChannelFeatureExtractor); tokens per clip = streams * frames
    conv_prefixes: Sequence[str] = ("extract_audio.cnn.",)   # state_dict prefix of every stream's stack (one entry: shared weights)
    ln_eps: float = 1e-6    # transformer layers (reference types/wavjepa_configs.py:37)
    norm_eps: float = 1e-5  # feature_norms / final norms (nn.LayerNorm default)
    norm_first_enc: bool = False   # pre-norm layers x = x + branch(LN(x)) in the student AND the teacher (nn.TransformerEncoderLayer norm_first)
    norm_first_dec: bool = False   # ... in the predictor
    conv_mode: str = "default"     # "default": GroupNorm on conv layer 0 only; "layer_norm": LayerNorm over channels behind EVERY conv layer
    conv_bias: bool = False        # conv layers carry a bias (mode "layer_norm" only)
    loss_kind: str = "mse"         # per-element loss of the masked objective: "mse" | "l1" | "smooth_l1" | "huber" (ops.masked_loss)
    loss_beta: float = 1.0         # smooth-L1's beta / Huber's delta
    recompute: bool = False        # activation recomputation in the student and the predictor (JEPA use_gradient_checkpointing; _alloc_ring)
    dropout_enc: float = 0.0       # dropout rate of the student's layers in a training-mode forward (never the teacher's); JepaEngine._drop
    dropout_dec: float = 0.0       # ... of the predictor's
    act_enc: str = "gelu"          # feed-forward activation of the student AND the teacher: "gelu" | "relu" | "gelu_tanh" | "silu" (ops.gemm_act)
    act_dec: str = "gelu"          # ... of the predictor
    layerdrop_enc: float = 0.0     # LayerDrop rate of the student's layers (never the teacher's): the kept lists come with each forward (_kept_now)
    layerdrop_dec: float = 0.0     # ... of the predictor's


class _Layer:
    """Raw device pointers of one transformer layer (weights bf16, biases / LN params fp32, gradients fp32)."""
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2", "g1", "be1", "g2", "be2",
                 "gwqkv", "gbqkv", "gwo", "gbo", "gw1", "gb1", "gw2", "gb2", "gg1", "gbe1", "gg2", "gbe2",
                 "wqkv_name", "wo_name", "w1_name", "w2_name",      # parameter names of the weights (student stacks)
                 "wqkvT", "woT", "w1T", "w2T",                      # bf16 W^T shadows (row-form dgrads), when the engine keeps them
                 "skip", "g_all")       # every parameter of the layer is frozen: the g* pointers read 0 (g_all keeps them, in _G_FIELDS' order)


_G_FIELDS = ("gwqkv", "gbqkv", "gwo", "gbo", "gw1", "gb1", "gw2", "gb2", "gg1", "gbe1", "gg2", "gbe2")


def _layer_ptrs(flat: FlatParams, prefix: str, teacher: bool) -> _Layer:
    L = _Layer()
    names = dict(wqkv="self_attn.in_proj_weight", bqkv="self_attn.in_proj_bias", wo="self_attn.out_proj.weight",
                 bo="self_attn.out_proj.bias", w1="linear1.weight", b1="linear1.bias", w2="linear2.weight",
                 b2="linear2.bias", g1="norm1.weight", be1="norm1.bias", g2="norm2.weight", be2="norm2.bias")
    for k, n in names.items():
        full = prefix + n
        is_w = k.startswith("w")
        if teacher:
            setattr(L, k, flat.tptr16(full) if is_w else flat.tptr32(full))
            setattr(L, "g" + k, 0)
        else:
            setattr(L, k, flat.ptr16(full) if is_w else flat.ptr32(full))
            setattr(L, "g" + k, flat.gptr(full))
            if is_w:
                setattr(L, k + "_name", full)
    L.skip, L.g_all = False, tuple(getattr(L, k) for k in _G_FIELDS)
    return L


class _Acts:
    """Saved activations of one transformer layer."""
    __slots__ = ("qkv", "o", "lse", "p", "m1", "r1", "x1", "x1b", "h", "g", "f", "m2", "r2", "x2", "x2b")


class EncoderEngine:
    # The trainable stacks, in the order a step's tables list them: per stack (slots of the backward's buffer ring, layers per grouped
    # weight-gradient launch), and the module that holds its parameters.  Stack s reads EngineConfig's d_s, h_s, l_s, norm_first_s,
    # dropout_s and act_s.
    BW_RING = dict(enc=(4, 2))
    MODULE = dict(enc="encoder")

    def __init__(self, cfg: EngineConfig, flat: FlatParams, pos_enc: torch.Tensor):
        ops.require_gpu()
        self.cfg, self.flat = cfg, flat
        self.dev = flat.device
        # fp32 tables on this device are used in place (load_state_dict / the data-parallel broadcast write through); a converted copy
        # (other dtype or device) is refreshed from its source in prepare_weights
        self.pos_enc = pos_enc.reshape(-1, cfg.d_enc).contiguous().float().to(self.dev)
        self._pos_src = [(self.pos_enc, pos_enc)]      # (the engine's table, its source)
        self.S = max(1, int(cfg.streams))            # channel streams through mono conv stacks
        self.stacks = list(cfg.conv_prefixes)        # distinct conv stacks; stream c uses stacks[min(c, len - 1)]
        assert len(self.stacks) in (1, self.S)
        self.C = cfg.conv_spec[-1][0]
        assert all(c == self.C for c, _, _ in cfg.conv_spec), "all conv layers must have the same width"
        if cfg.conv_mode not in ("default", "layer_norm"):
            raise ValueError(f"conv_mode must be 'default' or 'layer_norm', not {cfg.conv_mode!r}")
        # mode="layer_norm": Conv1d(+bias) -> LayerNorm over channels -> GELU in every conv layer (csrc/conv_ln.hip)
        self.conv_ln = cfg.conv_mode == "layer_norm"
        if cfg.conv_bias and not self.conv_ln:
            raise NotImplementedError("conv_bias=True needs mode='layer_norm': the GroupNorm front-end's kernels carry no conv bias")
        if self.conv_ln and self.C not in (64, 128, 256, 512):
            raise NotImplementedError(f"mode='layer_norm' runs conv widths 64 / 128 / 256 / 512, not {self.C}")
        # audio -> post[-1] and back: geometry, conv buffers, weight layouts, forward and backward walkers (conv_frontend.py)
        self.front = ConvFrontend(cfg.conv_spec, cfg.in_channels, cfg.n_samples, self.S, self._conv_params(), self.conv_ln, self.dev)
        self.L, self.P = self.front.L, self.front.P
        self.Tc = self.L[-1]                         # conv frames per stream
        self.T = self.S * self.Tc                    # tokens per clip: channel-major "B (C S)" flatten
        assert all(getattr(cfg, "d_" + s) % getattr(cfg, "h_" + s) == 0 for s in self.BW_RING)
        # clips of more than 416 tokens run the block-streamed attention kernels (ops.attn_entries), which take 32- and 64-wide heads
        if self.T > ops.ATTN_STREAM_T_MAX:
            raise NotImplementedError(f"{self.T} tokens per clip: the attention kernels take at most {ops.ATTN_STREAM_T_MAX}")
        # dropout (nn.TransformerEncoderLayer's four sites) in the trainable stacks of a training-mode forward: the _drop entries,
        # whose masks are a function of (drop_seed, drop_call, stack, layer, site, element) -- nothing is stored, the backward and the
        # second forward of recompute mode pass the same tail again.  The attention of such a stack runs the streamed family at any length.
        checks = [(self.MODULE[s], getattr(cfg, "dropout_" + s), getattr(cfg, "norm_first_" + s),
                   getattr(cfg, "d_" + s) // getattr(cfg, "h_" + s), getattr(cfg, "l_" + s)) for s in self.BW_RING]
        for what, _, _, hd, layers in checks:
            if self.T > ops.ATTN_WHOLE_T_MAX and layers > 0 and hd not in (32, 64):
                raise NotImplementedError(f"{self.T} tokens per clip with {hd}-wide {what} heads: attention beyond "
                                          f"{ops.ATTN_WHOLE_T_MAX} tokens (wj_attn_stream_fwd / _bwd) takes head widths 32 and 64")
        for what, p, pre, hd, layers in checks:
            if not (0.0 <= float(p) < 1.0):
                raise ValueError(f"{what} dropout must lie in [0, 1), not {p}")
            if p > 0 and pre:
                raise NotImplementedError(f"{what}: dropout={p} with norm_first=True: the dropout kernels cover post-norm layers only")
            if p > 0 and layers > 0 and hd not in (32, 64):
                raise NotImplementedError(f"{what}: dropout={p} with {hd}-wide heads: attention dropout runs in the streamed kernels "
                                          "(wj_attn_stream_fwd_drop / _bwd_drop), which take head widths 32 and 64")
        for s in self.BW_RING:
            if not (0.0 <= float(getattr(cfg, "layerdrop_" + s)) < 1.0):
                raise ValueError(f"{self.MODULE[s]} layerdrop must lie in [0, 1), not {getattr(cfg, 'layerdrop_' + s)}")
        self.drop_seed, self.drop_call = 0, 0
        # LayerDrop: stack -> the sorted indices of the layers that run in the training forward being run and in its backward (a stack
        # that is not named runs every layer).  Everything positional in the walkers (_stack_fwd, _stack_bwd, _redo_layer) follows the
        # position in this list, everything that names a layer its entry.
        self._kept_now: Dict[str, List[int]] = {}
        self._drop_now: Dict[str, float] = {}          # stack -> rate, for the forward being run and its backward ({}: no dropout)
        # the arena (alloc): clips, sequences per stack, whether it holds the training buffers, rows of every stack's buffers
        self.N, self.seqs, self._train_alloc = 0, {}, False
        for s in self.BW_RING:
            setattr(self, "cap_" + s, 0)
        self.audio = None       # the clips of the forward being run (the conv backward reads them again)
        # second HIP stream: work that is off the critical path (teacher forward; all weight-gradient GEMMs of the
        # backward) runs beside the main chain and fills the tails / write bursts of its kernels (WJ_SIDE_STREAM=0: off)
        self.use_side = os.environ.get("WJ_SIDE_STREAM", "1") != "0"
        self._opt_ev = self._opt_main = None    # a parameter update in flight on the side stream, the compute stream it was issued from
        # conv backward over the active rows only (needs a ragged step and k >= stride in every GEMM conv layer)
        self.sparse_conv = os.environ.get("WJ_SPARSE_CONV", "1") != "0" and all(k >= st for _, k, st in cfg.conv_spec[1:])
        # deterministic mode (WJ_DETERMINISTIC=1, or engine.deterministic = True before a step): every float sum of the backward whose
        # order follows arrival order by default -- the split-K weight gradients, the column-sum folds, the attention backward's LDS
        # sums -- takes its store-and-sum form (include/wavjepa_hip.h: the `deterministic` fields).  Loss, gradients, parameters and Adam
        # moments are then bit-identical from run to run on one build and GPU model.  The slabs of the split-K forms live in two
        # scratch buffers, one per stream (_det_ws), allocated once.
        self.deterministic = os.environ.get("WJ_DETERMINISTIC", "0") == "1"
        self._det_slab: Dict[str, torch.Tensor] = {}
        # GELU' of conv layers 1..n-2 in the epilogue of the sparse dgrad above them (WJ_FUSE_CONV_GELU_BWD=0: separate passes)
        self.fuse_conv_gelu_bwd = os.environ.get("WJ_FUSE_CONV_GELU_BWD", "1") != "0"
        # MX fp8 forward GEMMs (BASELINE config 5; build-defined numerics, WJ_FP8=1 or engine.fp8 = True): every transformer forward
        # linear whose K is a multiple of 256 runs on block-scaled e4m3 operands (wj_gemm_mxfp8, 2x the bf16 MFMA rate); weights are
        # re-quantised from their bf16 shadows once per step, activations by wj_quantize_mxfp8 in front of each GEMM.  The backward
        # is unchanged: it differentiates the bf16 graph (straight-through), with the saved bf16 activations and bf16 weights.
        self.fp8 = os.environ.get("WJ_FP8", "0") == "1"
        # activation recomputation (EngineConfig.recompute): a layer of the student / predictor keeps only the output the next layer reads;
        # everything else it saves lives in a ring of the backward's slot count and is computed again in front of the layer's backward
        self.recompute = bool(cfg.recompute)
        self._check_fp8()
        self._w8: Dict[int, Tuple[torch.Tensor, torch.Tensor, int, int]] = {}     # bf16 weight pointer -> (q, scales, N, K)
        self._a8: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}               # per stack: activation scratch (q, scales)
        self.side = self._pick_side_stream() if self.use_side else torch.cuda.Stream(device=self.dev)
        self.has_mapper = "post_extraction_mapper.weight" in flat.by_name
        # dgrads dx = dy . W as ROW-form GEMMs against bf16 W^T shadows of the transformer weights (refreshed once per step by one
        # batched transpose, wj_transpose_bf16): the persistent eight-phase kernel instead of the col-form 256 x 128 schedule.
        # WJ_WT_DGRAD=0 keeps the col-form dgrads (A/B runs).
        self.wt_dgrad = os.environ.get("WJ_WT_DGRAD", "1") != "0"
        # K-split pairs for the student's 117-tile GEMMs (scratch handed to the main-stream launches of that stack).  Round 6: OFF by default
        # (WJ_PAIR_SPLIT=1 enables) -- on the two-stream step they move nothing (46.85 / 46.87 ms in round 5, 46.09 with / 46.02 without in
        # round 6, interleaved on one box) while costing 30 MB of partial sums per launch (traffic 1.31 x algorithmic) and a spin-wait between
        # workgroups; a one-stream host (WJ_SIDE_STREAM=0) gains 0.3 ms with them.  One default for both, so that the serialised profile
        # measures the kernels the timed step runs.
        self.pair_split = os.environ.get("WJ_PAIR_SPLIT", "0") == "1"
        self.pair_ws = None
        self.defer_folds = os.environ.get("WJ_DEFER_FOLDS", "1") != "0"
        self.fuse_add_pos = os.environ.get("WJ_FUSE_ADD_POS", "1") != "0"     # 0: mapper GEMM + wj_add_pos as two launches
        self.mapper_wgrad_side = os.environ.get("WJ_MAPPER_WGRAD_SIDE", "1") != "0"
        self.conv_wgrad_side = os.environ.get("WJ_CONV_WGRAD_SIDE", "1") != "0"   # 0: the sparse conv weight gradients on the main stream
        # LayerNorm forward in its LEAN form on a capped grid (wj_ln_fwd_args.workgroups; csrc/norm.hip) for the stacks named in WJ_LN_LEAN
        # ("tea", "enc", "dec", joined by + or ,; default: none): a kernel of <= 48 VGPRs shares a CU with the persistent GEMM workgroups of
        # the OTHER stream (teacher beside student / predictor).  Measured (round 6, interleaved, one box): 45.79 ms/step without, 47.05 with
        # all three, 45.91 teacher only, 47.63 student + predictor only, 45.94 with a cap of 1024 -- a capped LayerNorm alone on its stream's
        # critical path loses more than it hides (DESIGN_EXPERIMENTS.md); off.  WJ_LN_LEAN_WGS: the cap (256 = one workgroup per CU).
        lean = os.environ.get("WJ_LN_LEAN", "")
        self.ln_lean = {t.strip() for t in lean.replace("+", ",").split(",") if t.strip() and t.strip() != "0"} if self.use_side else set()
        self.ln_lean_wgs = int(os.environ.get("WJ_LN_LEAN_WGS", "256"))
        self._lean_now = False                 # set inside the training forward only: inference runs one stream, nothing to stream under
        self._folds = []
        # partial training (freeze.py; set_frozen): the frozen parameter names the step was last told of, the units all of whose
        # parameters are frozen (no parameter-gradient launch), per backward section the elements of partly frozen units that are
        # cleared behind it, and whether an accumulation window has been opened by a backward since the buffer was last clear
        self._frozen: frozenset = frozenset()
        self._skip: frozenset = frozenset()
        self._clear_ranges: Dict[str, List[Tuple[int, int]]] = {}
        self._frozen_memo: Dict[frozenset, tuple] = {}
        self._accum_open = False
        self.grad_mult = 1.0             # feature_grad_mult in (0, 1]: the factor on d(post[-1]) in front of the conv backward (0: frozen)
        self._bind_params()
        self._bind_wt()

    def _pick_side_stream(self) -> torch.cuda.Stream:
        """A second stream that really runs beside the current one.  HIP deals streams onto a few hardware queues round-robin;
        two streams on one queue serialise (measured: with a process group active RCCL's streams shift the deal and the
        side stream landed on the main stream's queue -- the whole two-stream overlap was gone).  Probe: one busy-wait
        wave on each stream, started together; concurrent streams take one wait, serialised ones two."""
        main = torch.cuda.current_stream(self.dev)
        ticks = 20000                                    # s_memtime ticks; calibrated below to a ~0.2 ms wait
        ops.spin(100, stream=main.cuda_stream)           # load the code object before timing

        def pair_ms(cand: torch.cuda.Stream) -> float:   # uses the calibrated `ticks`
            e0, e1, go, done = (torch.cuda.Event(enable_timing=True) for _ in range(4))
            best = 1e9
            for _ in range(2):
                go.record(main)
                cand.wait_event(go)
                e0.record(main)
                ops.spin(ticks, stream=main.cuda_stream)
                ops.spin(ticks, stream=cand.cuda_stream)
                done.record(cand)
                main.wait_event(done)
                e1.record(main)
                e1.synchronize()
                best = min(best, e0.elapsed_time(e1))
            return best

        def single_ms() -> float:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(main)
            ops.spin(ticks, stream=main.cuda_stream)
            e1.record(main)
            e1.synchronize()
            return e0.elapsed_time(e1)

        single = single_ms()
        if single < 0.15:                                # faster tick than assumed: stretch the wait to ~0.2 ms
            ticks = int(ticks * 0.2 / max(single, 1e-3))
            single = single_ms()
        cands = [torch.cuda.Stream(device=self.dev) for _ in range(6)] + [torch.cuda.Stream(device=self.dev, priority=-1)]
        self._stream_probe = []
        for cand in cands:
            t = pair_ms(cand)
            self._stream_probe.append(round(t / max(single, 1e-6), 2))
            if t < 1.5 * single:
                return cand
        return cands[0]                                  # nothing overlapped: keep the semantics, lose the overlap

    # ------------------------------------------------------------------------------------------------ parameters
    def _bind_params(self) -> None:
        for s, module in self.MODULE.items():
            setattr(self, s + "_layers", [_layer_ptrs(self.flat, f"{module}.layers.{i}.", False) for i in range(getattr(self.cfg, "l_" + s))])

    def _conv_params(self) -> List[List[ConvLayerParams]]:
        """[stack][layer] parameter and gradient pointers of the conv stacks (layer 0: bf16 weight; layers 1..: the fp32 master)."""
        f, c = self.flat, self.cfg
        norm = "2.1." if self.conv_ln else "2."          # Sequential(-, LayerNorm, -) behind every conv / GroupNorm behind conv 0

        def layer(pre: str, l: int) -> ConvLayerParams:
            w, b = f"{pre}{l}.0.weight", f"{pre}{l}.0.bias" if c.conv_bias else None
            g, be = (f"{pre}{l}.{norm}weight", f"{pre}{l}.{norm}bias") if self.conv_ln or l == 0 else (None, None)
            ptr, gptr = (lambda n: None if n is None else f.ptr32(n)), (lambda n: None if n is None else f.gptr(n))
            return ConvLayerParams(f.ptr16(w) if l == 0 else f.ptr32(w), ptr(b), ptr(g), ptr(be), gptr(w), gptr(b), gptr(g), gptr(be))
        return [[layer(pre, l) for l in range(len(c.conv_spec))] for pre in self.stacks]

    def set_frozen(self, frozen) -> None:
        """The frozen parameter names of the step about to run (a training-mode forward and its backward).  A layer all of whose
        parameters are frozen hands 0 for every gradient pointer -- the norm and attention backwards then fold nothing, the dgrad
        epilogue sums no columns -- and queues no weight gradient; the other units are asked through _skipped().  The frozen names of
        a partly frozen unit are cleared behind their section of the backward (_clear_frozen).  An open accumulation window holds
        sums made under the old set: ValueError."""
        frozen = frozenset(frozen)
        if frozen == self._frozen:
            return
        if self._accum_open and not self.flat.g_clean:
            raise ValueError("the frozen set changed inside an open gradient-accumulation window: freeze / unfreeze between optimiser steps")
        if frozen not in self._frozen_memo:          # (a schedule or a loop that alternates sets pays the name arithmetic once per set)
            from . import freeze
            names = [s.name for s in self.flat.slots]
            by_tag: Dict[str, set] = {}
            for name in freeze.partly_frozen(names, frozen):
                by_tag.setdefault(freeze.section_of(name, self.cfg.l_enc), set()).add(name)
            self._frozen_memo[frozen] = (freeze.skipped_units(names, frozen), {tag: self.flat.ranges_of(part) for tag, part in by_tag.items()})
        self._frozen = frozen
        self._skip, self._clear_ranges = self._frozen_memo[frozen]
        for s, module in self.MODULE.items():
            for i, w in enumerate(self._stack(s)[0]):
                w.skip = f"{module}.layers.{i}" in self._skip
                for k, g in zip(_G_FIELDS, w.g_all):
                    setattr(w, k, 0 if w.skip else g)
        self.flat.set_frozen(frozen)

    def _skipped(self, unit: str) -> bool:
        return unit in self._skip

    def _clear_frozen(self, tag: Optional[str]) -> None:
        """Zero the frozen elements of partly frozen units whose gradients section `tag` of the backward made final (None: all of
        them), on the calling stream: one fill per merged range.  No launch when nothing is partly frozen."""
        for t, ranges in self._clear_ranges.items():
            if tag is None or t == tag:
                for lo, hi in ranges:
                    self.flat.g32[lo:hi].zero_()

    def _bind_wt(self) -> None:
        """W^T shadows: one more bf16 buffer with the parameter layout, every 2-D transformer weight stored transposed at its own offset."""
        f, trained = self.flat, [w for s in self.BW_RING for w in self._stack(s)[0]]
        self._enc_ids = {id(w) for w in self.enc_layers}       # the student's layers (their main-stream launches carry the K-split scratch)
        self.p16t = None
        self._wt_tables = {}                   # (per stack: its weights that take the row form) -> (table, n_mats, n_tiles)
        self._wt_need = ()                     # ... of the step being run (set by the forward from its row counts)
        if self.wt_dgrad:
            ok = all(r % 64 == 0 and cc % 64 == 0 for w in trained for k in ("wqkv", "wo", "w1", "w2")
                     for r, cc in [f.by_name[getattr(w, k + "_name")].shape])
            if ok:
                self.p16t = torch.zeros(f.n, dtype=torch.bfloat16, device=self.dev)
                for w in trained:
                    for k in ("wqkv", "wo", "w1", "w2"):
                        setattr(w, k + "T", self.p16t.data_ptr() + 2 * f.by_name[getattr(w, k + "_name")].offset)
            else:
                self.wt_dgrad = False          # a width that is not a multiple of 64: keep the col-form dgrads
        self._wt_fresh = None                  # the `_wt_need` the shadows were last refreshed for (None: stale)
        self._wt_live = {}

    @staticmethod
    def _row_form_pays(M: int, N: int) -> bool:
        """A dgrad [M, N] takes the row form (W^T shadow) only where it fills the persistent kernel: >= 256 work items of 256 rows x
        256 / 128 columns.  Measured in the step, the student's 117-tile dgrads (M ~ 10 k context rows, N = 768) run 58 / 47 / 20 us in
        col form on the 256 x 128 schedule (234 workgroups) against 64 / 49 / 24 us in row form on the one-tile eight-phase schedule."""
        return -(-M // 256) * (N // 256 + (1 if N % 256 else 0)) >= 256

    PAIR_TILES = (33, 128)      # output tiles of a problem that runs as K-split pairs (csrc/gemm.hip: pair_shape)

    def _pair_pays(self, M: int, N: int, K: int) -> bool:
        """A row-form GEMM [M, N] over K that the library runs as K-split pairs when it is handed scratch (wj_gemm_args.workspace): the
        ragged student's N = 768 products (117 tiles for 256 CUs).  Measured (tools/gemm_small.py, operands not cache-resident):
        K = 3072 74 -> 60 us, K = 2304 58 -> 48 us, against 75 / 57 us for the col-form dgrad; K = 768 loses (27 -> 30 us)."""
        tiles = -(-M // 256) * (N // 256)
        return self.pair_split and N % 256 == 0 and K % 256 == 0 and K >= 1536 and self.PAIR_TILES[0] <= tiles <= self.PAIR_TILES[1]

    def _wt_keys(self, M: int, D: int, pairs: bool = False):
        """The weights of a stack of width D whose dgrad over M rows takes the row form (output widths: w2 -> 4D, the others -> D;
        contraction lengths: wqkv 3D, wo D, w1 4D, w2 D).  pairs: the stack's launches carry the K-split scratch (the student)."""
        if not self.wt_dgrad:
            return ()
        return tuple(k for k, n_out, k_in in (("wqkv", D, 3 * D), ("wo", D, D), ("w1", D, 4 * D), ("w2", 4 * D, D))
                     if self._row_form_pays(M, n_out) or (pairs and self._pair_pays(M, n_out, k_in)))

    def _check_fp8(self) -> None:
        if self.fp8 and (self.cfg.act_enc != "gelu" or self.cfg.act_dec != "gelu"):
            raise RuntimeError(f"fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with activation={self.cfg.act_enc!r} (encoder) / "
                               f"{self.cfg.act_dec!r} (decoder): the MX fp8 forward GEMM (wj_gemm_mxfp8) has the erf-GELU epilogue only")
        if self.fp8 and (self.cfg.dropout_enc > 0 or self.cfg.dropout_dec > 0):
            raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with dropout > 0: the fp8 producers (LayerNorm and GELU "
                               "epilogues that emit the next GEMM's operand) have no dropout forms")
        if self.fp8 and (self.cfg.layerdrop_enc > 0 or self.cfg.layerdrop_dec > 0):
            raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with layerdrop > 0 (encoder_layerdrop / decoder_layerdrop): "
                               "a layer hands its output to the next one in the stack's fp8 scratch, and nothing pins that hand-over "
                               "across a skipped layer")
        if self.fp8 and self.recompute:
            # the fp8 forward hands a layer's output to the next layer in the stack's fp8 scratch as well; a second forward that starts
            # from a kept bf16 output would quantise it in another launch order, and nothing pins that to the first pass's bits
            raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with activation recomputation (recompute=True / "
                               "use_gradient_checkpointing): the second forward runs in bf16")
        if self.fp8 and (self.cfg.norm_first_enc or self.cfg.norm_first_dec):
            raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) covers post-norm stacks only: a norm_first=True stack runs in bf16")
        if self.fp8 and self.cfg.conv_mode == "layer_norm":
            raise RuntimeError("fp8 mode (WJ_FP8=1 / engine.fp8) is not combined with the mode='layer_norm' conv front-end")

    def _fwd_stacks(self) -> List[Tuple[List[_Layer], int]]:
        """(layers, width) of every stack a forward runs, in the order their fp8 weights are quantised."""
        return [self._stack(s)[:2] for s in self.BW_RING]

    def _fp8_weights(self) -> None:
        """(Re-)quantise the forward weights of the transformer stacks from their bf16 shadows (once per step in fp8 mode)."""
        self._check_fp8()
        if not self._w8:
            for layers, d in self._fwd_stacks():
                for w in layers:
                    for ptr, n, k in ((w.wqkv, 3 * d, d), (w.wo, d, d), (w.w1, 4 * d, d), (w.w2, d, 4 * d)):
                        if k % 256 == 0:
                            self._w8[ptr] = (_empty(n, k, dtype=torch.uint8, device=self.dev),
                                             torch.zeros(ops.fp8_scale_dwords(n, k), dtype=torch.int32, device=self.dev), n, k)
        for ptr, (q, sc, n, k) in self._w8.items():
            ops.quantize_mxfp8(ptr, q, sc, M=n, K=k, ldx=k, ldq=k, ld_scale=n)

    def _linear_fwd(self, stack: str, x, w_ptr: int, out, *, M: int, N: int, K: int, bias, epilogue: int = ops.EPI_BF16, C2=None,
                    act: str = "gelu") -> None:
        """out[M, N] = x[M, K] . W^T (+ bias, epilogue): the bf16 GEMM, or in fp8 mode (eligible K) quantise x and run the MX fp8 GEMM.
        act (linear1's two calls): another activation than GELU in the epilogue's place -- ops.gemm_act, never in fp8 mode (_check_fp8)."""
        if act != "gelu":
            ops.gemm_act(x, w_ptr, out, act=act, C2=C2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=epilogue)
            return
        w8 = self._w8.get(w_ptr) if self.fp8 else None
        if w8 is None:
            ops.gemm(x, w_ptr, out, C2=C2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=epilogue,
                     workspace=self.pair_ws if stack == "enc" else None)       # K-split pairs: main-stream launches only
            return
        q, sc = self._a8[stack]
        ops.quantize_mxfp8(x, q, sc, M=M, K=K, ldx=K, ldq=K, ld_scale=M)
        ops.gemm_mxfp8(q, w8[0], sc, w8[1], out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ld_scale_a=M, ld_scale_b=N, epilogue=epilogue,
                       C2=C2, bias=bias)

    def prepare_weights(self, force_cast: bool = False) -> None:
        """bf16 shadow copies (when stale) + the GEMM layouts of conv layers 1.. from the fp32 masters."""
        f = self.flat
        if force_cast or not f.bf16_fresh or self.fp8:
            self.wait_optimizer()
        for mine, src in self._pos_src:
            if mine.data_ptr() != src.data_ptr():
                mine.copy_(src.reshape(mine.shape))
        if force_cast or not f.bf16_fresh:
            ops.cast_f32_to_bf16(f.p32, f.p16, f.n)
            if f.tn > 0:
                ops.cast_f32_to_bf16(f.t32, f.t16, f.tn)
            f.bf16_fresh = True
        if self.fp8:
            self._fp8_weights()
        self._wt_fresh = None                       # the shadows follow p16; refreshed by the first backward that needs them
        self.front.w_fresh = False                  # GEMM layouts of conv layers 1..: rebuilt by the front-end, behind its conv0 launches

    # ------------------------------------------------------------------------------------------------ arena
    def _alloc_stack(self, M: int, D: int, H: int, B: int, layers: int, skip: Sequence[str] = ()) -> List[_Acts]:
        """`layers` sets of everything a layer saves for its backward; the buffers named in `skip` are left out (None)."""
        bf, f32 = torch.bfloat16, torch.float32
        shapes = dict(qkv=((M, 3 * D), bf), o=((M, D), bf), lse=((B * H * self.T,), f32), p=((M, D), bf), m1=((M,), f32), r1=((M,), f32),
                      x1=((M, D), f32), x1b=((M, D), bf),
                      h=((M, 4 * D), bf),           # holds gelu'(linear1 output), see EPI_BIAS_GELU2
                      g=((M, 4 * D), bf), f=((M, D), bf), m2=((M,), f32), r2=((M,), f32), x2=((M, D), f32), x2b=((M, D), bf))
        assert tuple(shapes) == _Acts.__slots__
        out = []
        for _ in range(layers):
            a = _Acts()
            for name, (shape, dtype) in shapes.items():
                setattr(a, name, None if name in skip else _empty(*shape, dtype=dtype, device=self.dev))
            out.append(a)
        return out

    def _alloc_ring(self, stack: str, M: int, B: int):
        """Recompute mode: (ring, kept, view) of a stack.  ring: as many full activation sets as the backward's buffer ring has slots
        (BW_RING), without the two buffers that are kept.  kept[i]: what layer i + 1 (or the final norm) reads of layer i, for every
        layer -- post-norm x2 (fp32) and x2b (bf16), pre-norm the stream x2 (fp32) and the branch output f (bf16) that the next norm
        adds: 6 D bytes per row.  view[i]: layer i's _Acts, slot i % nbuf of the ring with kept[i] in place of the two buffers, which
        is what the layer forms and their backward are handed in either pass."""
        layers, D, H, pre, _ = self._stack(stack)
        nbuf = self.BW_RING[stack][0]
        names = ("x2", "f") if pre else ("x2", "x2b")
        ring = self._alloc_stack(M, D, H, B, min(nbuf, len(layers)), skip=names)
        kept, view = [], []
        for i in range(len(layers)):
            kept.append((_empty(M, D, dtype=torch.float32, device=self.dev), _empty(M, D, dtype=torch.bfloat16, device=self.dev)))
            v = _Acts()
            for name in _Acts.__slots__:
                setattr(v, name, getattr(ring[i % nbuf], name))
            setattr(v, names[0], kept[i][0])
            setattr(v, names[1], kept[i][1])
            view.append(v)
        return ring, kept, view

    def _acts(self, stack: str) -> List[_Acts]:
        """Per layer of the stack: where it saves for the backward (recompute mode: ring slot + kept output, _alloc_ring)."""
        return getattr(self, stack + ("_view" if self.recompute else "_acts"))

    def alloc(self, N: int, train: bool = True, seqs: Optional[Dict[str, int]] = None, **need: int) -> None:
        """(Re)build the arena for N clips.  seqs: sequences per batch of every trainable stack other than "enc" (which has N).

        need_<stack>: rows that stack's buffers must hold this step (a ragged step: its context / visible rows; a dense step: every
        token of every sequence; 0 = dense).  A stack's activations and backward scratch, and the buffers its step engine sizes
        with it, follow that need + WJ_ARENA_MARGIN (default 15 %), not the dense worst case: with the AudioSet masker a
        ragged step touches 19 % / 42 % of the dense rows, and those buffers were 57 of the 86 GB of a 256-clip arena.  A later step
        that needs more (a batch with more visible tokens, the dense fall-back, WJ_RAGGED=0) grows them -- a re-allocation, rare by
        construction.  WJ_ARENA_DENSE=1 sizes everything for the dense step up front."""
        seqs = dict(seqs or {}, enc=N)
        full = {s: seqs[s] * self.T for s in self.BW_RING}
        if os.environ.get("WJ_ARENA_DENSE", "0") == "1" or not train:
            need = {}
        rows = {s: min(need.get("need_" + s) or full[s], full[s]) for s in full}
        same = N == self.N and (not train or (self._train_alloc and seqs == self.seqs))
        if same and (not train or all(rows[s] <= getattr(self, "cap_" + s) for s in full)):
            return
        margin = float(os.environ.get("WJ_ARENA_MARGIN", "1.15"))
        for s in full:
            old = getattr(self, "cap_" + s) if same else 0
            setattr(self, "cap_" + s, full[s] if rows[s] >= full[s] else min(full[s], max((int(rows[s] * margin) + 255) // 256 * 256, old)))
        self.N, self.seqs, self.M, self._train_alloc = N, seqs, N * self.T, train
        self._arena(N, train)

    def _alloc_a8(self, tag: str, m: int, d: int) -> None:
        """fp8 mode: the activation scratch (e4m3 bytes + block scales) of one stack, m rows of width d"""
        dev = self.dev
        self._a8[tag] = (_empty(m, 4 * d, dtype=torch.uint8, device=dev), torch.zeros(ops.fp8_scale_dwords(m, 4 * d), dtype=torch.int32, device=dev))
        self._a8s[tag] = (_empty(m, d, dtype=torch.uint8, device=dev), torch.zeros(ops.fp8_scale_dwords(m, d), dtype=torch.int32, device=dev))

    def _arena(self, N: int, train: bool) -> None:
        """The buffers of the front-end and of every trainable stack (a step engine adds its own behind them)."""
        c, bf, f32, dev = self.cfg, torch.bfloat16, torch.float32, self.dev
        M, C = self.M, self.C
        self.front.alloc(N, train)                    # conv activations, statistics and their gradients
        if self.pair_split and self.pair_ws is None:
            # zero-filled ONCE; the library keeps its flags at zero between launches.  Sized for the largest problem that splits.
            self.pair_ws = torch.zeros(ops.workspace_bytes("wj_gemm_bf16", M=256 * (self.PAIR_TILES[1] // 2), N=512, K=2048, lda=2048, ldb=2048,
                                                           ldc=512, epilogue=ops.EPI_BF16), dtype=torch.uint8, device=dev)
        self.fn_b = _empty(M, C, dtype=bf, device=dev)
        self.fn_mean = _empty(M, dtype=f32, device=dev)
        self.fn_rstd = _empty(M, dtype=f32, device=dev)
        self.map_b = _empty(M, c.d_enc, dtype=bf, device=dev)
        self.lf = _empty(M, c.d_enc, dtype=f32, device=dev)
        self.lf_b = _empty(M, c.d_enc, dtype=bf, device=dev)
        # 'enc' is sized for all M rows even when the student's activation buffers follow the ragged row count: infer() runs the
        # student stack densely (M rows) on whatever arena a training step left behind (N == self.N skips alloc), and the quantiser /
        # GELU q_out epilogue write M x 4D bytes into this scratch -- with cap_enc rows that was an out-of-bounds device write
        self._a8, self._a8s = {}, {}
        self._alloc_a8("enc", M, c.d_enc)
        # scratch stack (inference; a frozen stack beside the student): one layer's worth, reused
        self.scratch = self._alloc_stack(M, c.d_enc, c.h_enc, N, 1)[0]
        self.enc_out = _empty(M, c.d_enc, dtype=f32, device=dev)
        self.enc_out_b = _empty(M, c.d_enc, dtype=bf, device=dev)
        self.enc_fm = _empty(M, dtype=f32, device=dev)
        self.enc_fr = _empty(M, dtype=f32, device=dev)
        if not train:
            return
        self.bw = {}                                  # backward scratch, one set per stack
        red = [ops.workspace_bytes("wj_layernorm_bwd", D=max([C] + [self._stack(s)[1] for s in self.BW_RING]))]
        for s, (nbuf, group) in self.BW_RING.items():
            layers, d, h, pre, _ = self._stack(s)
            m, B = getattr(self, "cap_" + s), self.seqs[s]    # rows of the stack's buffers (<= its dense rows)
            if self.recompute:
                acts, kept, view = self._alloc_ring(s, m, B)
                setattr(self, s + "_kept", kept)
                setattr(self, s + "_view", view)
            else:
                acts = self._alloc_stack(m, d, h, B, len(layers))
            setattr(self, s + "_acts", acts)
            # a pre-norm stack: the stream that enters its final norm (its backward needs it; post-norm reads the last layer's x2)
            setattr(self, s + "_sf", _empty(m, d, dtype=f32, device=dev) if pre else None)
            # The weight gradients of `group` consecutive layers go out as ONE grouped launch on the side stream (wj_wgrad_grouped:
            # one small split-K factor for 4-8 problems instead of a large one per problem).  The buffers it reads (dY of every
            # linear) therefore exist 2 * group times (slot = layer % nbuf), so that the main chain may run a whole group ahead.
            self.bw[s] = dict(
                dy=_empty(m, d, dtype=f32, device=dev), ds=_empty(m, d, dtype=f32, device=dev),
                dx1=_empty(m, d, dtype=f32, device=dev), do=_empty(m, d, dtype=bf, device=dev),
                dgb=_empty(m, d, dtype=bf, device=dev), dxb=_empty(m, d, dtype=bf, device=dev),   # bf16 grad_input of linear1 / in_proj
                dsb2=[_empty(m, d, dtype=bf, device=dev) for _ in range(nbuf)],
                dsb1=[_empty(m, d, dtype=bf, device=dev) for _ in range(nbuf)],
                dh=[_empty(m, 4 * d, dtype=bf, device=dev) for _ in range(nbuf)],
                dqkv=[_empty(m, 3 * d, dtype=bf, device=dev) for _ in range(nbuf)],
                done=[torch.cuda.Event() for _ in range(nbuf)], used=[False] * nbuf, nbuf=nbuf, group=group, pending=[], pending_slots=[])
            red.append(ops.workspace_bytes("wj_attn_bwd", B=B, H=h, hd=d // h))
        # scratch for two-stage parameter-gradient reductions (LayerNorm: [1536][3][D]; attention in_proj bias: [B][3D])
        red_bytes = max(red)
        self.red_ws = _empty(red_bytes // 4, dtype=f32, device=dev)
        # deferred folds (WJ_DEFER_FOLDS=0: every LayerNorm / attention backward folds its own partials at once, 75 launches of ~5 us
        # per step): each pending producer keeps its partial rows in its own slot until one grouped launch folds up to 16 of them
        self._red_bytes = (red_bytes + 255) // 256 * 256
        self.fold_ws = _empty(ops.COLSUM_GROUP_MAX * self._red_bytes // 4, dtype=f32, device=dev)
        self._folds = []
        self.d_lf_b = _empty(M, c.d_enc, dtype=bf, device=dev)
        self.d_fn = _empty(M, C, dtype=f32, device=dev)

    # ------------------------------------------------------------------------------------------------ building blocks
    # ---- pieces of a layer that the post-norm and the pre-norm layout share
    def _drop(self, stack: str, layer: int, site: int):
        """The dropout tail (ops.drop_args) of one site of one layer, or None when the stack runs without dropout in this forward."""
        p = self._drop_now.get(stack, 0.0)
        if not p:
            return None
        return ops.drop_args(self.drop_seed, self.drop_call, p, site=site, layer=layer, stack=ops.DROP_STACK[stack])

    def _attn_fwd(self, a: _Acts, D: int, H: int, B: int, mask: Optional[torch.Tensor], seq: Optional[Tuple[torch.Tensor, int]],
                  save: bool, drop=None) -> None:
        """a.o = attention(a.qkv): packed sequences (`seq`) or T tokens per sequence under a key mask; `save` keeps the softmax statistics.
        drop: dropout on the probabilities (the streamed family, at any length)."""
        lse = a.lse if save else None
        if drop is not None:
            kw = dict(T=seq[1], seq_off=seq[0]) if seq is not None else dict(T=self.T, key_mask=mask)
            ops.attn_stream_fwd_drop(a.qkv, a.o, B=B, H=H, hd=D // H, lse=lse, drop=drop, **kw)
        elif seq is not None:
            fwd = getattr(ops, ops.attn_entries(seq[1])[0][3:])      # by the length bound of THIS call: a short ragged stack keeps the whole-image kernels
            fwd(a.qkv, a.o, B=B, T=seq[1], H=H, hd=D // H, seq_off=seq[0], lse=lse)
        else:
            fwd = getattr(ops, ops.attn_entries(self.T)[0][3:])
            fwd(a.qkv, a.o, B=B, T=self.T, H=H, hd=D // H, key_mask=mask, lse=lse)

    def _tail_gather(self, a: _Acts, x: torch.Tensor, sub: Tuple[torch.Tensor, torch.Tensor, int], D: int):
        """The `sub` rows of the attention output and of the residual source x: (tail_o, tail_x, the number of rows that go on).
        (tail_o / tail_x / tail_do belong to the arena of the step engine that passes `sub`.)"""
        rows, _, M = sub
        ops.mask_gather_rows(a.o, rows, self.tail_o, n_rows=M, D=D, elem_bytes=2)
        ops.mask_gather_rows(x, rows, self.tail_x, n_rows=M, D=D, elem_bytes=4)
        return self.tail_o, self.tail_x, M

    def _mlp_fwd(self, stack: str, w: _Layer, a: _Acts, xb: torch.Tensor, M: int, D: int, save: bool, out: bool = True, drop=None) -> None:
        """a.f = linear2(gelu(linear1(xb))) in bf16; `save` also keeps gelu'(linear1 output) in a.h for the backward.
        out=False: linear1 only (a.g and a.h), for a second forward whose a.f was kept from the first.
        drop: dropout behind the GELU, one pass over a.g and a.h with the same mask -- linear2's weight gradient (reads a.g) and the
        MUL_GELU_GRAD dgrad epilogue (reads a.h) are then correct as they stand."""
        act = getattr(self.cfg, "act_" + stack, self.cfg.act_enc)               # (a frozen stack runs the encoder's activation)
        if save:
            self._linear_fwd(stack, xb, w.w1, a.h, M=M, N=4 * D, K=D, bias=w.b1, epilogue=ops.EPI_BIAS_GELU2, C2=a.g, act=act)
        else:
            self._linear_fwd(stack, xb, w.w1, a.g, M=M, N=4 * D, K=D, bias=w.b1, epilogue=ops.EPI_BIAS_GELU, act=act)
        if drop is not None:
            ops.dropout_rows(a.g, a.h if save else None, M=M, N=4 * D, drop=drop)
        if out:
            self._linear_fwd(stack, a.g, w.w2, a.f, M=M, N=D, K=4 * D, bias=w.b2)

    def _layer_fwd(self, w: _Layer, a: _Acts, x_in: torch.Tensor, xb_in: torch.Tensor, M: int, D: int, H: int, B: int,
                   mask: Optional[torch.Tensor], seq: Optional[Tuple[torch.Tensor, int]] = None, save: bool = True,
                   x2_out: Optional[torch.Tensor] = None, x2_stats: Optional[torch.Tensor] = None,
                   sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, stack: str = "enc", xq_ready: bool = False,
                   redo: bool = False, li: int = 0) -> bool:
        """Post-norm layer: x1 = LN1(x + out_proj(attn(in_proj(x)))); x2 = LN2(x1 + linear2(gelu(linear1(x1)))).
        `seq` = (offsets int32 [B+1], longest sequence) selects the ragged form: M packed rows, no key mask.
        save=False (teacher / inference): nothing is kept for a backward (no gelu' output, no softmax statistics).
        sub = (rows int32 [Ms], inverse int32 [M], Ms): only these rows continue after the attention (the last predictor layer:
        context rows are keys / values there and nothing reads their outputs).
        xq_ready / return value (fp8 mode): the stack's small fp8 buffer already / now holds this layer's input / output.
        redo (recompute mode, in front of the layer's backward): the same launches once more; x2 / x2b were kept from the first pass --
        the side stream may be reading x2b -- so norm2 writes its row statistics only.
        li: the layer's index in its stack (the dropout masks' layer field)."""
        eps = self.cfg.ln_eps
        if self._drop_now.get(stack):
            return self._layer_fwd_drop(w, a, x_in, xb_in, M, D, H, B, mask, seq, sub, stack, redo, li)
        # fp8 mode with an eligible width (K = D a multiple of 256): the GEMM inputs are produced directly in the MX fp8 operand
        # format by their producers -- LayerNorm (x1 for linear1, x2 for the next layer's in_proj) and linear1's GELU epilogue
        # (for linear2); only the attention output and the very first layer input go through wj_quantize_mxfp8
        f8 = self.fp8 and w.wqkv in self._w8
        if not f8:
            xq_ready = False
            self._linear_fwd(stack, xb_in, w.wqkv, a.qkv, M=M, N=3 * D, K=D, bias=w.bqkv)
        else:
            qb, sb = self._a8[stack]             # [M][4D] bytes: gelu(h)
            qs, ss = self._a8s[stack]            # [M][D] bytes: x2 -> attention output -> x1 -> x2 (one stream: strictly sequential)
            if not xq_ready:
                ops.quantize_mxfp8(xb_in, qs, ss, M=M, K=D, ldx=D, ldq=D, ld_scale=M)
            self._gemm8(qs, ss, w.wqkv, a.qkv, M=M, N=3 * D, K=D, bias=w.bqkv)
        self._attn_fwd(a, D, H, B, mask, seq, save)
        o_in = a.o
        if sub is not None:
            o_in, x_in, M = self._tail_gather(a, x_in, sub, D)
        f8_out = dict(y_fp8=qs, y_fp8_scales=ss, ld_fp8_scale=M) if f8 else {}
        if f8:
            ops.quantize_mxfp8(o_in, qs, ss, M=M, K=D, ldx=D, ldq=D, ld_scale=M)
            self._gemm8(qs, ss, w.wo, a.p, M=M, N=D, K=D, bias=w.bo)
        else:
            self._linear_fwd(stack, o_in, w.wo, a.p, M=M, N=D, K=D, bias=w.bo)
        lean = self.ln_lean_wgs if (self._lean_now and stack in self.ln_lean and not f8) else 0
        ops.layernorm_fwd(x_in, w.g1, w.be1, M=M, D=D, eps=eps, r=a.p, y_f32=a.x1, y_bf16=a.x1b, mean=a.m1, rstd=a.r1, workgroups=lean, **f8_out)
        if f8:
            gq = dict(q_out=qb, q_scales=sb, ld_q_scale=M)
            if save:
                self._gemm8(qs, ss, w.w1, a.h, M=M, N=4 * D, K=D, bias=w.b1, epilogue=ops.EPI_BIAS_GELU2, C2=a.g, **gq)
            else:                                              # teacher / inference: gelu(h) exists in fp8 only
                self._gemm8(qs, ss, w.w1, None, M=M, N=4 * D, K=D, bias=w.b1, epilogue=ops.EPI_BIAS_GELU, **gq)
            self._gemm8(qb, sb, w.w2, a.f, M=M, N=D, K=4 * D, bias=w.b2)
        else:
            self._mlp_fwd(stack, w, a, a.x1b, M, D, save)
        # x2_out / x2_stats (teacher): the layer output goes to its own buffer and its per-clip (sum, sum of squares) is
        # accumulated on the way, so that the targets are ONE pass over the kept layers (wj_instnorm_mean)
        y2 = (None, None) if redo else (a.x2 if x2_out is None else x2_out, a.x2b)
        ops.layernorm_fwd(a.x1, w.g2, w.be2, M=M, D=D, eps=eps, r=a.f, y_f32=y2[0], y_bf16=y2[1],
                          mean=a.m2, rstd=a.r2, group_stats=x2_stats, group_rows=self.T if x2_stats is not None else 0,
                          workgroups=lean if x2_stats is None else 0, **f8_out)
        return f8 and sub is None              # the small fp8 buffer now holds x2 for the next layer of this stack

    def _layer_fwd_drop(self, w: _Layer, a: _Acts, x_in, xb_in, M: int, D: int, H: int, B: int, mask, seq, sub, stack: str, redo: bool,
                        li: int) -> bool:
        """_layer_fwd of a student / predictor layer under dropout (always saving, never fp8): the same GEMMs; the attention and the two
        residual LayerNorms in their _drop forms, and one pass over linear1's outputs."""
        eps = self.cfg.ln_eps
        self._linear_fwd(stack, xb_in, w.wqkv, a.qkv, M=M, N=3 * D, K=D, bias=w.bqkv)
        self._attn_fwd(a, D, H, B, mask, seq, True, drop=self._drop(stack, li, ops.DROP_SITE_ATTN))
        o_in = a.o
        if sub is not None:
            o_in, x_in, M = self._tail_gather(a, x_in, sub, D)
        self._linear_fwd(stack, o_in, w.wo, a.p, M=M, N=D, K=D, bias=w.bo)
        ops.layernorm_fwd_drop(x_in, w.g1, w.be1, M=M, D=D, eps=eps, r=a.p, y_f32=a.x1, y_bf16=a.x1b, mean=a.m1, rstd=a.r1,
                               drop=self._drop(stack, li, ops.DROP_SITE_RES1))
        self._mlp_fwd(stack, w, a, a.x1b, M, D, True, drop=self._drop(stack, li, ops.DROP_SITE_FFN))
        y2 = (None, None) if redo else (a.x2, a.x2b)
        ops.layernorm_fwd_drop(a.x1, w.g2, w.be2, M=M, D=D, eps=eps, r=a.f, y_f32=y2[0], y_bf16=y2[1], mean=a.m2, rstd=a.r2,
                               drop=self._drop(stack, li, ops.DROP_SITE_RES2))
        return False

    def _layer_fwd_pre(self, w: _Layer, a: _Acts, x_in, r_in, M: int, D: int, H: int, B: int, mask: Optional[torch.Tensor],
                       seq: Optional[Tuple[torch.Tensor, int]] = None, save: bool = True, s_out: Optional[torch.Tensor] = None,
                       s_stats: Optional[torch.Tensor] = None, sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                       stack: str = "enc", redo: bool = False):
        """Pre-norm layer (norm_first=True): s1 = s0 + out_proj(attn(in_proj(LN1(s0)))); s2 = s1 + linear2(gelu(linear1(LN2(s1)))).
        The residual add of a branch is fused into the NEXT norm (wj_layernorm_pre_fwd), so the layer takes its input as the pair
        (x_in, r_in) -- s0 = x_in + r_in, r_in = the previous layer's linear2 output, None for the first layer of a stack -- and returns
        its output as the pair (s1, linear2 output): the next layer's norm1, or the stack's final norm, adds them.
        Saved in `a`: x1 = s0 (when r_in is None, s0 is x_in itself and nothing is stored), x1b = LN1(s0), x2 = s1, x2b = LN2(s1).
        s_out / s_stats (teacher): s0 -- the previous layer's output -- goes to its own buffer, with its per-clip (sum, sum of squares).
        seq, save, sub: as _layer_fwd.  redo (recompute mode, in front of the layer's backward): the same launches once more, without
        the two outputs that were kept from the first pass (x2 is not written again, linear2 is not run: no backward reads a.f)."""
        eps = self.cfg.ln_eps
        s0 = x_in if (r_in is None and s_out is None) else (a.x1 if s_out is None else s_out)
        ops.layernorm_pre_fwd(x_in, w.g1, w.be1, M=M, D=D, eps=eps, r=r_in, s_f32=None if s0 is x_in else s0, y_bf16=a.x1b,
                              mean=a.m1 if save else None, rstd=a.r1 if save else None, group_stats=s_stats,
                              group_rows=self.T if s_stats is not None else 0)
        self._linear_fwd(stack, a.x1b, w.wqkv, a.qkv, M=M, N=3 * D, K=D, bias=w.bqkv)
        self._attn_fwd(a, D, H, B, mask, seq, save)
        o_in = a.o
        if sub is not None:
            o_in, s0, M = self._tail_gather(a, s0, sub, D)
        self._linear_fwd(stack, o_in, w.wo, a.p, M=M, N=D, K=D, bias=w.bo)
        ops.layernorm_pre_fwd(s0, w.g2, w.be2, M=M, D=D, eps=eps, r=a.p, s_f32=None if redo else a.x2, y_bf16=a.x2b,
                              mean=a.m2 if save else None, rstd=a.r2 if save else None)
        self._mlp_fwd(stack, w, a, a.x2b, M, D, save, out=not redo)
        return a.x2, a.f

    def _gemm8(self, q, sc, w_ptr: int, out, *, M: int, N: int, K: int, bias, epilogue: int = ops.EPI_BF16, C2=None, **extra) -> None:
        w8 = self._w8[w_ptr]
        ops.gemm_mxfp8(q, w8[0], sc, w8[1], out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, ld_scale_a=M, ld_scale_b=N, epilogue=epilogue, C2=C2,
                       bias=bias, **extra)

    def set_wt_need(self, *rows: int) -> None:
        """Which weights' dgrads run in row form this step (decided per stack, in BW_RING's order, from its row count)."""
        stacks = [(s == "enc",) + self._stack(s)[:2] for s in self.BW_RING]
        self._wt_need = tuple(self._wt_keys(m, d, pairs=student) if layers else () for (student, layers, d), m in zip(stacks, rows))
        self._wt_live = {id(w): keys for (_, layers, _), keys in zip(stacks, self._wt_need) for w in layers}

    def refresh_wt(self) -> None:
        """bf16 W^T shadows from the current bf16 weights: one batched transpose of the weights this step's dgrads read in row form
        (`_wt_need`: with the AudioSet masker at 256 clips all four of every predictor layer and linear2 of every student layer,
        99 of the 213 MB of transformer weights); once per prepared set of weights."""
        need = self._wt_need
        # fresh only for the set of weights it was refreshed for: a second grad-enabled forward on the same prepared weights with other
        # row counts (direct engine use, gradient accumulation) needs other shadows, which would still hold zeros / older weights
        if not self.wt_dgrad or self._wt_fresh == need:
            return
        if need not in self._wt_tables:
            f, rows, tiles = self.flat, [], 0
            for layers, keys in zip((self._stack(s)[0] for s in self.BW_RING), need):
                for w in layers:
                    for k in keys:
                        sl = f.by_name[getattr(w, k + "_name")]
                        r, cc = sl.shape
                        rows.append((sl.offset, r, cc, tiles))
                        tiles += (r // 64) * (cc // 64)
            self._wt_tables[need] = (torch.tensor(rows, dtype=torch.int64, device=self.dev) if rows else None, len(rows), tiles)
        table, n_mats, n_tiles = self._wt_tables[need]
        if n_mats:
            ops.transpose_bf16(self.flat.p16, self.p16t, table, n_mats, n_tiles)
        self._wt_fresh = need

    def _dgrad(self, dY, w: _Layer, key: str, out, *, M: int, N: int, K: int, **kw) -> None:
        """out[M, N] = dY[M, K] . W   (W = the layer's `key` weight, stored [K][N] as nn.Linear keeps it): against the W^T shadow as a
        row-form GEMM, or (WJ_WT_DGRAD=0, widths that are not multiples of 64) against W itself in col form."""
        colsum = kw.get("colsum") if self.deterministic else None
        if colsum is not None:
            # the fused column sums meet in one float atomic per row tile: deterministic mode sums the bf16 output in a pass of its own
            kw = {k: v for k, v in kw.items() if k != "colsum"}
        self._dgrad_gemm(dY, w, key, out, M=M, N=N, K=K, **kw)
        if colsum is not None:
            self._colsum_bf16(out, colsum, M=M, N=N, ldx=N)

    def _dgrad_gemm(self, dY, w: _Layer, key: str, out, *, M: int, N: int, K: int, **kw) -> None:
        if self.wt_dgrad and key in self._wt_live.get(id(w), ()):
            ops.gemm(dY, getattr(w, key + "T"), out, M=M, N=N, K=K, lda=K, ldb=K, ldc=N,
                     workspace=self.pair_ws if id(w) in self._enc_ids else None, **kw)
        else:
            ops.gemm(dY, getattr(w, key), out, M=M, N=N, K=K, lda=K, ldb=N, ldc=N, b_trans=1, **kw)

    # ---- parameter-gradient folds of the LayerNorm / attention backward, deferred and grouped
    def _fold_slot(self) -> int:
        if len(self._folds) >= ops.COLSUM_GROUP_MAX:
            self._flush_folds()
        return self.fold_ws.data_ptr() + len(self._folds) * self._red_bytes

    def _flush_folds(self) -> None:
        """One launch adds the column sums of every pending partial matrix to its gradient slices (stream-ordered behind the
        kernels that wrote them; called before a section of the gradient buffer is declared final).  (On the side stream, with two
        scratch buffers: 46.64 against 46.65 ms/step -- stays on the main stream.)"""
        if self._folds:
            if self.deterministic:
                ops.colsum_f32_group(self._folds, deterministic=True)
            else:
                ops.colsum_f32_group(self._folds)
            self._folds = []

    # ---- deterministic mode: scratch and call forms
    def _det_ws_bytes(self) -> Tuple[int, int]:
        """(slab bytes, column-sum partial bytes) that cover every deterministic launch of a step, from the library's own queries: the
        split factor of a weight gradient grows with its K (the token rows) up to a limit set by its shapes, so K = 2^30 asks for
        that limit -- one size for every mask draw, no allocation inside a step."""
        need, big = 0, 1 << 30
        widths = [self._stack(s)[1] for s in self.BW_RING]
        for d, (_, group) in zip(widths, self.BW_RING.values()):
            layer = [(0, 0, 0, d, 4 * d, big), (0, 0, 0, 4 * d, d, big), (0, 0, 0, d, d, big), (0, 0, 0, 3 * d, d, big)]
            for n in range(1, group + 1):
                need = max(need, ops.wgrad_grouped_workspace_bytes(layer * n))
        for m, n in self._split_wgrad_shapes():
            need = max(need, ops.workspace_bytes("wj_gemm_bf16", M=m, N=n, K=big, ldc=n, a_trans=1, b_trans=1, epilogue=ops.EPI_ATOMIC_F32,
                                                 split_k=ops.pick_split_k(m, n, big), deterministic=1))
        cs = max(ops.workspace_bytes("wj_colsum_bf16", M=big, N=n, deterministic=1) for d in widths for n in (d, 4 * d))
        return need, cs

    def _split_wgrad_shapes(self) -> List[Tuple[int, int]]:
        """[n_out, k_in] of the weight gradients that go out as single split-K GEMMs (_wgrad; the conv layers')"""
        return [(self.cfg.d_enc, self.C)] + [(self.C, k * self.C) for _, k, _ in self.cfg.conv_spec[1:]]

    def _det_ws(self) -> torch.Tensor:
        """The slab scratch of the stream the caller launches on: the main stream and the side stream each own one, so two weight
        gradients in flight never share a slab (launches of one stream are ordered)."""
        if not self._det_slab:
            slab, cs = self._det_ws_bytes()
            for tag in ("main", "side"):
                self._det_slab[tag] = _empty(max(slab, 256), dtype=torch.uint8, device=self.dev)
            self._det_slab["colsum"] = _empty(max(cs, 256) // 4, dtype=torch.float32, device=self.dev)     # main-stream launches only
        on_side = self.use_side and torch.cuda.current_stream() == self.side
        return self._det_slab["side" if on_side else "main"]

    def _det_kw(self) -> dict:
        """extra arguments of a split-K weight-gradient ops.gemm call (none by default: the call is then exactly the default one)"""
        return dict(workspace=self._det_ws(), deterministic=True) if self.deterministic else {}

    def _colsum_bf16(self, x, out, *, M: int, N: int, ldx: int) -> None:
        if self.deterministic:
            self._det_ws()
            ops.colsum_bf16(x, out, M=M, N=N, ldx=ldx, workspace=self._det_slab["colsum"], deterministic=True)
        else:
            ops.colsum_bf16(x, out, M=M, N=N, ldx=ldx)

    def _fold_form(self, N: int, wanted: bool, defer: bool = True, fits: bool = True):
        """How the partial rows [rows][N] of a kernel's parameter gradients get folded into the gradient buffer -> (form, scratch):
        "slot": the kernel leaves them in a slot of fold_ws, folded later with the neighbours' by one grouped launch (_flush_folds);
        "now":  deterministic mode without a slot: the kernel leaves them in red_ws, folded in order at once;
        "own":  the kernel reduces by itself (no scratch from here), or no gradient output was asked for (`wanted`).
        defer=False: a producer that never waits for the grouped fold; fits: its partial rows fit a slot."""
        if wanted and defer and self.defer_folds and N <= 2304 and fits:
            return "slot", self._fold_slot()
        if wanted and self.deterministic:
            return "now", self.red_ws
        return "own", None

    def _fold(self, form: str, ws, N: int, rows: int, o0, o1, o2, n_each: int) -> None:
        """queue ("slot") or perform ("now") the fold of the partial rows a kernel left in `ws`"""
        if form == "slot":
            self._folds.append((ws, N, rows, N, o0, o1, o2, n_each))
        elif form == "now" and N > 2304:
            raise RuntimeError(f"deterministic mode: no ordered fold for {N} columns (wj_colsum_f32_group takes <= 2304)")
        elif form == "now":          # deterministic fold of one partial matrix, at once (the undeferred forms)
            ops.colsum_f32_group([(ws, N, rows, N, o0, o1, o2, n_each)], deterministic=True)

    def _ln_bwd(self, dy, x, gamma, mean, rstd, *, M: int, D: int, dgamma=None, dbeta=None, dbias=None, defer: bool = True,
                workspace=None, drop=None, **kw) -> None:
        """wj_layernorm_bwd; its dgamma / dbeta / dbias partials are folded later, together with the neighbours' (see _flush_folds), or
        in deterministic mode at once -- never by the kernel's own atomics then.  workspace: what an undeferred caller hands the
        kernel's own reduction (a deferring one: red_ws)."""
        wanted = bool(dgamma or dbeta or dbias)      # (none: a skipped unit -- no partial rows, no fold slot)
        form, ws = self._fold_form(3 * D, wanted, defer)
        ln_bwd = ops.layernorm_bwd
        if drop is not None:         # the addend r went through dropout: wj_layernorm_bwd_drop, the same partial rows
            ln_bwd, kw = ops.layernorm_bwd_drop, dict(kw, drop=drop)
        if form == "own":
            ln_bwd(dy, x, gamma, mean, rstd, M=M, D=D, dgamma=dgamma, dbeta=dbeta, dbias=dbias,
                   workspace=(self.red_ws if defer else workspace) if wanted else None, **kw)
        else:
            ln_bwd(dy, x, gamma, mean, rstd, M=M, D=D, workspace=ws, **kw)
            self._fold(form, ws, 3 * D, ops.ln_bwd_partial_rows(M, D), dgamma, dbeta, dbias, D)

    def _ln_pre_bwd(self, dy, s, gamma, mean, rstd, *, M: int, D: int, dgamma=None, dbeta=None, dbias=None, **kw) -> None:
        """wj_layernorm_pre_bwd with the fold forms of _ln_bwd."""
        wanted = bool(dgamma or dbeta or dbias)
        form, ws = self._fold_form(3 * D, wanted)
        if form == "own":
            ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, M=M, D=D, dgamma=dgamma, dbeta=dbeta, dbias=dbias,
                                  workspace=self.red_ws if wanted else None, **kw)
        else:
            ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, M=M, D=D, workspace=ws, **kw)
            self._fold(form, ws, 3 * D, ops.ln_pre_bwd_partial_rows(M, D), dgamma, dbeta, dbias, D)

    def _attn_bwd(self, qkv, out, dout, lse, dqkv, *, B: int, H: int, hd: int, dbias, drop=None, **kw) -> None:
        """wj_attn_bwd (wj_attn_stream_bwd above 416 tokens, the same arguments and the same [B][3D] partial rows): the in_proj bias partials
        go to a slot, or the kernel folds them itself out of red_ws (in order when deterministic)."""
        D3 = 3 * H * hd
        attn_bwd = getattr(ops, ops.attn_entries(kw["T"])[1][3:])
        if drop is not None:         # dropout on the probabilities: the streamed family at any length
            attn_bwd, kw = ops.attn_stream_bwd_drop, dict(kw, drop=drop)
        if self.deterministic:
            kw = dict(kw, deterministic=True)
        form, ws = self._fold_form(D3, bool(dbias))
        if form == "slot":
            attn_bwd(qkv, out, dout, lse, dqkv, B=B, H=H, hd=hd, dbias=dbias, dbias_ws=ws, defer_fold=True, **kw)
            self._fold(form, ws, D3, B, dbias, None, None, D3)
        else:
            attn_bwd(qkv, out, dout, lse, dqkv, B=B, H=H, hd=hd, dbias=dbias, dbias_ws=self.red_ws, **kw)

    def _wgrad(self, dY, X, gW, n_out: int, k_in: int, m_tok: int) -> None:
        """gW[n_out, k_in] += dY[m_tok, n_out]^T @ X[m_tok, k_in]   (the three mapper weights: nothing on the main chain reads the result, so
        the launch goes to the side stream -- WJ_MAPPER_WGRAD_SIDE=0: main stream)"""
        def go():
            ops.gemm(dY, X, gW, M=n_out, N=k_in, K=m_tok, lda=n_out, ldb=k_in, ldc=k_in, a_trans=1, b_trans=1,
                     epilogue=ops.EPI_ATOMIC_F32, split_k=ops.pick_split_k(n_out, k_in, m_tok), **self._det_kw())
        if self.use_side and self.mapper_wgrad_side:
            self._on_side(go)
        else:
            go()

    def _on_side(self, fn) -> None:
        """Run `fn` (kernel launches) on the side stream after everything enqueued so far on the main stream."""
        if not self.use_side:
            fn()
            return
        main = torch.cuda.current_stream()
        ev = torch.cuda.Event()
        ev.record(main)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            fn()

    def optimizer_on_side(self, fn) -> None:
        """The parameter update of everything the front-end does not read, on the side stream behind everything the compute stream has
        queued (gradient norm, the front-end parameters' update); the compute stream waits for it in wait_optimizer()."""
        self._opt_main = torch.cuda.current_stream()       # the compute stream the update was issued from
        self._on_side(fn)
        self._opt_ev = torch.cuda.Event()
        self._opt_ev.record(self.side)

    def wait_optimizer(self) -> None:
        """The calling stream waits for a parameter update still in flight on the side stream (no host wait).  Called by the forward in front
        of its first transformer kernel, by inference, the EMA, weight preparation, state_dict, Module._apply and at the end of Trainer.fit.
        The event is kept until the COMPUTE stream (the one the update was issued from) has waited: a first caller on some other stream
        (a state_dict inside a `torch.cuda.stream(...)` block) must not consume it for the next forward."""
        if self._opt_ev is not None:
            cur = torch.cuda.current_stream()
            cur.wait_event(self._opt_ev)
            if self._opt_main is None or cur == self._opt_main:
                self._opt_ev = None

    def _join_side(self) -> None:
        if self.use_side:
            ev = torch.cuda.Event()
            ev.record(self.side)
            torch.cuda.current_stream().wait_event(ev)

    # ---- pieces of a layer's backward that the post-norm and the pre-norm layout share
    def _slot_wait(self, bw: dict, slot: int) -> None:
        if self.use_side and bw["used"][slot]:
            torch.cuda.current_stream().wait_event(bw["done"][slot])   # side stream finished reading this slot's buffers

    def _mlp_bwd(self, w: _Layer, a: _Acts, xb: torch.Tensor, bw: dict, parity: int, M: int, D: int) -> None:
        """d(linear2 output) (bf16, bw["dsb2"][parity]) -> d(linear1 input) (bf16, bw["dgb"]); xb: the bf16 operand linear1 read.
        The two weight gradients are queued (_wgrads)."""
        dsb2, dh = bw["dsb2"][parity], bw["dh"][parity]
        self._dgrad(dsb2, w, "w2", dh, M=M, N=4 * D, K=D, epilogue=ops.EPI_MUL_GELU_GRAD, aux=a.h,
                    colsum=w.gb1 or None)        # linear1.bias gradient = column sums of dh, fused into the producing epilogue
        if not w.skip:                   # (a layer all of whose parameters are frozen: no weight gradient)
            bw["pending"] += [(dsb2, a.g, w.gw2, D, 4 * D, M), (dh, xb, w.gw1, 4 * D, D, M)]
        self._dgrad(dh, w, "w1", bw["dgb"], M=M, N=D, K=4 * D)

    def _attn_block_bwd(self, w: _Layer, a: _Acts, xb: torch.Tensor, bw: dict, parity: int, M: int, D: int, H: int, B: int,
                        mask: Optional[torch.Tensor], seq: Optional[Tuple[torch.Tensor, int]],
                        sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]], drop=None) -> torch.Tensor:
        """d(out_proj output) (bf16, bw["dsb1"][parity]; with `sub`: on the sub-rows) -> d(qkv) over all M rows (bw["dqkv"][parity]);
        xb: the bf16 operand in_proj read.  Returns the fp32 residual gradient over all M rows: bw["ds"], with `sub` scattered into
        bw["dx1"].  The two weight gradients are queued (_wgrads)."""
        ds, dx1, do, dsb1, dqkv = bw["ds"], bw["dx1"], bw["do"], bw["dsb1"][parity], bw["dqkv"][parity]
        if sub is None:
            Ms, o_in, ds_all = M, a.o, ds
            self._dgrad(dsb1, w, "wo", do, M=M, N=D, K=D)
        else:                             # back to all rows: zero gradient where no output was used
            Ms, o_in, ds_all = sub[2], self.tail_o, dx1
            self._dgrad(dsb1, w, "wo", self.tail_do, M=Ms, N=D, K=D)
            ops.unmask_rows_f32(self.tail_do, sub[1], do, M=M, D=D, dst_is_bf16=True)
            ops.unmask_rows_f32(ds, sub[1], dx1, M=M, D=D, src_is_f32=True)       # dx1 is free again: residual gradient
        if seq is not None:
            self._attn_bwd(a.qkv, a.o, do, a.lse, dqkv, B=B, T=seq[1], H=H, hd=D // H, seq_off=seq[0], dbias=w.gbqkv, drop=drop)
        else:
            self._attn_bwd(a.qkv, a.o, do, a.lse, dqkv, B=B, T=self.T, H=H, hd=D // H, key_mask=mask, dbias=w.gbqkv, drop=drop)
        if not w.skip:
            bw["pending"] += [(dsb1, o_in, w.gwo, D, D, Ms), (dqkv, xb, w.gwqkv, 3 * D, D, M)]
        return ds_all

    def _wgrads(self, bw: dict, parity: int, flush: bool) -> None:
        """The four weight-gradient GEMMs of a layer only need (dY, X) and nothing downstream needs them before the optimiser: they are
        queued, and with `flush` the queue goes out as grouped launches on the side stream while the main stream continues the dgrad
        chain (`parity` = the layer's buffer slot; its `done` event tells the main stream when the slot may be written again)."""
        bw["pending_slots"].append(parity)
        if not flush:
            return
        probs, slots = bw["pending"], bw["pending_slots"]
        bw["pending"], bw["pending_slots"] = [], []

        def wgrads():
            for i in range(0, len(probs), 8):
                if self.deterministic:
                    ops.wgrad_grouped(probs[i:i + 8], workspace=self._det_ws(), deterministic=True)
                else:
                    ops.wgrad_grouped(probs[i:i + 8])
            if self.use_side:
                for sl in slots:
                    bw["done"][sl].record(self.side)
                    bw["used"][sl] = True
        self._on_side(wgrads)

    def _layer_bwd(self, w: _Layer, a: _Acts, x_in: torch.Tensor, xb_in: torch.Tensor, dy: torch.Tensor, dyb: Optional[torch.Tensor],
                   dx_out: torch.Tensor, M: int, D: int, H: int, B: int, mask: Optional[torch.Tensor], bw: dict, parity: int,
                   seq: Optional[Tuple[torch.Tensor, int]] = None,
                   sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, flush: bool = True, bottom: bool = False,
                   stack: str = "enc", li: int = 0, floor: bool = False):
        """d(x2) = dy (fp32) + dyb (bf16 or None) -> d(x_in), returned as (fp32 part, bf16 part or None, flushed); parameter gradients
        accumulated into the flat gradient buffer.
        The grad_input of linear1 and in_proj is what a bf16 linear returns under autocast -- a bf16 tensor (`dgb` / `dxb`) -- and the
        LayerNorm backward that consumes the sum adds it to the fp32 residual gradient on its way in (`dy2`): 2 + 2 bytes per element
        instead of the 4 + 4 of a read-modify-write fp32 GEMM epilogue.  Only the `bottom` layer of a stack folds the two into one
        fp32 tensor (dx_out), for the consumers below the stack.
        Returns flushed = True when the weight-gradient queue went out (_wgrads: the queued layers' gradients are then final in
        side-stream order).
        stack, li: which layer this is -- under dropout the two LayerNorm backwards and the attention backward regenerate the forward's
        masks from them (the FFN site needs nothing: a.g and a.h were stored masked).
        floor: nothing trainable lies below this layer (freeze.py): its own parameter gradients, no in_proj dgrad."""
        ds, dxb, dqkv = bw["ds"], bw["dxb"], bw["dqkv"][parity]
        if not self.recompute:             # (recompute mode: _redo_layer waited for the slot before it wrote the activations)
            self._slot_wait(bw, parity)
        Ms, x_ln1 = M, x_in
        if sub is not None:              # dy holds the sub-rows only; everything up to the attention works on them
            Ms, x_ln1 = sub[2], self.tail_x
        self._ln_bwd(dy, a.x1, w.g2, a.m2, a.r2, M=Ms, D=D, r=a.f, dy2=dyb, dy2_is_bf16=dyb is not None, ds_f32=ds, ds_bf16=bw["dsb2"][parity],
                     dgamma=w.gg2, dbeta=w.gbe2, dbias=w.gb2, drop=self._drop(stack, li, ops.DROP_SITE_RES2))
        self._mlp_bwd(w, a, a.x1b, bw, parity, Ms, D)
        self._ln_bwd(ds, x_ln1, w.g1, a.m1, a.r1, M=Ms, D=D, r=a.p, dy2=bw["dgb"], dy2_is_bf16=True, ds_f32=ds, ds_bf16=bw["dsb1"][parity],
                     dgamma=w.gg1, dbeta=w.gbe1, dbias=w.gbo, drop=self._drop(stack, li, ops.DROP_SITE_RES1))      # ds updated in place
        ds_all = self._attn_block_bwd(w, a, xb_in, bw, parity, M, D, H, B, mask, seq, sub, drop=self._drop(stack, li, ops.DROP_SITE_ATTN))
        self._wgrads(bw, parity, flush)
        if floor:
            return None, None, flush
        if bottom:
            self._dgrad(dqkv, w, "wqkv", dx_out, M=M, N=D, K=3 * D, epilogue=ops.EPI_ADD_F32, aux=ds_all)
            return dx_out, None, flush
        self._dgrad(dqkv, w, "wqkv", dxb, M=M, N=D, K=3 * D)
        return ds_all, dxb, flush

    def _layer_bwd_pre(self, w: _Layer, a: _Acts, s0: torch.Tensor, below: Optional[_Layer], dx_out: torch.Tensor, M: int, D: int, H: int,
                       B: int, mask: Optional[torch.Tensor], bw: dict, parity: int, seq: Optional[Tuple[torch.Tensor, int]] = None,
                       sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, flush: bool = True):
        """Backward of _layer_fwd_pre.  On entry bw["ds"] holds d(s2) (fp32) and bw["dsb2"][parity] its bf16 rounding -- both written by
        the backward of the norm one half-layer up (the layer above's norm1, or the stack's final norm), which also gave linear2.bias its
        gradient.  On exit the same holds for the layer `below` (slot parity - 1); below = None (the first layer of the stack): d(s0)
        goes to dx_out (fp32) for the consumers below the stack.  s0: the stream the layer read (a.x1, or the stack's input for the
        first layer).  Returns (d(s0) buffer, flushed)."""
        ds, dxb = bw["ds"], bw["dxb"]
        if not self.recompute:             # (recompute mode: waited for in front of the layer's second forward, see _redo_layer)
            self._slot_wait(bw, parity)
        Ms = M if sub is None else sub[2]      # ds holds the sub-rows only; everything up to the attention works on them
        self._mlp_bwd(w, a, a.x2b, bw, parity, Ms, D)
        # norm2: d(s1) = d(s2) + LN2'(d LN2(s1)), in place; its bf16 rounding is out_proj's dY, its column sums out_proj.bias's gradient
        self._ln_pre_bwd(bw["dgb"], a.x2, w.g2, a.m2, a.r2, M=Ms, D=D, dres=ds, dy_is_bf16=True, ds_f32=ds, ds_bf16=bw["dsb1"][parity],
                         dgamma=w.gg2, dbeta=w.gbe2, dbias=w.gbo)
        ds_all = self._attn_block_bwd(w, a, a.x1b, bw, parity, M, D, H, B, mask, seq, sub)
        self._wgrads(bw, parity, flush)
        self._dgrad(bw["dqkv"][parity], w, "wqkv", dxb, M=M, N=D, K=3 * D)
        # norm1: d(s0) = d(s1) + LN1'(d LN1(s0)).  Above a layer it is that layer's d(s2): fp32 in bw["ds"], bf16 (linear2's dY) in the
        # layer's own slot, column sums = its linear2.bias gradient -- every gradient of THIS layer is out when the call returns
        if below is None:
            self._ln_pre_bwd(dxb, s0, w.g1, a.m1, a.r1, M=M, D=D, dres=ds_all, dy_is_bf16=True, ds_f32=dx_out,
                             dgamma=w.gg1, dbeta=w.gbe1)
            return dx_out, flush
        pb = (parity - 1) % bw["nbuf"]
        self._slot_wait(bw, pb)              # (slot pb's last readers went out at least a layer ago)
        self._ln_pre_bwd(dxb, s0, w.g1, a.m1, a.r1, M=M, D=D, dres=ds_all, dy_is_bf16=True, ds_f32=ds, ds_bf16=bw["dsb2"][pb],
                         dgamma=w.gg1, dbeta=w.gbe1, dbias=below.gb2)
        return ds, flush

    # ---- a whole stack: the layers and the final norm, in either norm order
    def _stack(self, stack: str):
        """(layers, width, heads, norm_first, name of the final norm) of a trainable stack"""
        c = self.cfg
        return (getattr(self, stack + "_layers"), getattr(c, "d_" + stack), getattr(c, "h_" + stack), getattr(c, "norm_first_" + stack),
                self.MODULE[stack] + ".norm")

    def _stack_fwd(self, stack: str, x: torch.Tensor, xb: torch.Tensor, M: int, B: int, mask: Optional[torch.Tensor],
                   seq: Optional[Tuple[torch.Tensor, int]] = None, *, acts: Optional[List[_Acts]] = None,
                   sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None, lean: bool = False, **out) -> None:
        """Walk a stack's layers forward from the stream x (fp32; xb: its bf16 copy, which only post-norm layers read), then its final
        norm, which writes `out` (y_f32 / y_bf16 / mean / rstd).  mask, seq: as _layer_fwd; sub: the rows that go on behind the last
        layer's attention.  acts: where every layer saves for the backward; None (inference): nothing is saved, every layer runs in
        self.scratch.  lean: the post-norm final norm may take its capped-grid form (WJ_LN_LEAN names the stack).
        LayerDrop: a saving walk runs the layers of _kept(stack) only; the stream passes the others unchanged."""
        c, f = self.cfg, self.flat
        layers, D, H, pre, norm = self._stack(stack)
        save = acts is not None
        # LayerDrop: the layers that run, kept[0] < kept[1] < ...; layer kept[j] saves in acts[j] (inference runs every layer)
        kept = self._kept(stack) if save else range(len(layers))
        top = len(kept) - 1
        gamma, beta = f.ptr32(norm + ".weight"), f.ptr32(norm + ".bias")
        Mo = M if sub is None else sub[2]                      # rows that leave the stack
        if top < 0 and sub is not None:                        # no layer runs: the final norm reads the sub-rows of the stack's input
            ops.mask_gather_rows(x, sub[0], self.tail_x, n_rows=Mo, D=D, elem_bytes=4)
            x = self.tail_x
        if pre:
            r = None
            for j, i in enumerate(kept):
                x, r = self._layer_fwd_pre(layers[i], acts[j] if save else self.scratch, x, r, M, D, H, B, mask, seq, save=save,
                                           sub=sub if j == top else None, stack=stack)
            # the final norm also performs the last residual add; the stream it normalises is kept for its backward (with no layer
            # there is no add, and the stream is the stack's input itself)
            ops.layernorm_pre_fwd(x, gamma, beta, M=Mo, D=D, eps=c.norm_eps, r=r,
                                  s_f32=getattr(self, stack + "_sf") if save and top >= 0 else None, **out)
            return
        xq = False
        for j, i in enumerate(kept):
            a = acts[j] if save else self.scratch
            xq = self._layer_fwd(layers[i], a, x, xb, M, D, H, B, mask, seq, save=save, sub=sub if j == top else None, stack=stack,
                                 xq_ready=xq, li=i)
            x, xb = a.x2, a.x2b
        ops.layernorm_fwd(x, gamma, beta, M=Mo, D=D, eps=c.norm_eps,
                          workgroups=self.ln_lean_wgs if (lean and self._lean_now and stack in self.ln_lean) else 0, **out)

    def _kept(self, stack: str) -> Sequence[int]:
        """The layers of the stack that run in the training forward being run and its backward (LayerDrop), ascending: every layer
        unless the forward was handed a kept list."""
        kept = self._kept_now.get(stack)
        return range(len(self._stack(stack)[0])) if kept is None else kept

    def _redo_layer(self, stack: str, j: int, x0: torch.Tensor, xb0: torch.Tensor, M: int, B: int, mask: Optional[torch.Tensor],
                    seq: Optional[Tuple[torch.Tensor, int]], sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]]) -> None:
        """Recompute mode: the forward of the j-th layer that ran (layer _kept(stack)[j]; without LayerDrop layer j) once more, from the
        kept output of the one that ran before it (or the stack's input) into ring slot j % nbuf, with the masks, offsets and sub-rows
        of the first pass.  The slot's last readers are the grouped weight gradients of position j + nbuf on the side stream: the main
        stream waits for the event that guards the slot before it writes -- once per layer: the layer's backward, which waits for the
        same event with the flag off, does not wait again."""
        bw, acts = self.bw[stack], self._acts(stack)
        layers, D, H, pre, _ = self._stack(stack)
        kept = self._kept(stack)
        i = kept[j]
        if not (pre and j < len(kept) - 1):        # (pre-norm: the backward of the layer above waited for this slot to write its dsb2)
            self._slot_wait(bw, j % bw["nbuf"])
        lean_was, self._lean_now = self._lean_now, self.use_side      # (WJ_LN_LEAN: the LayerNorm form of the first pass)
        try:
            if pre:
                x, r = (x0, None) if j == 0 else (acts[j - 1].x2, acts[j - 1].f)
                self._layer_fwd_pre(layers[i], acts[j], x, r, M, D, H, B, mask, seq, save=True, sub=sub, stack=stack, redo=True)
            else:
                x, xb = (x0, xb0) if j == 0 else (acts[j - 1].x2, acts[j - 1].x2b)
                self._layer_fwd(layers[i], acts[j], x, xb, M, D, H, B, mask, seq, save=True, sub=sub, stack=stack, redo=True, li=i)
        finally:
            self._lean_now = lean_was

    def _stack_bwd(self, stack: str, x0: torch.Tensor, xb0: torch.Tensor, M: int, B: int, mask: Optional[torch.Tensor],
                   seq: Optional[Tuple[torch.Tensor, int]] = None, *, sub: Optional[Tuple[torch.Tensor, torch.Tensor, int]] = None,
                   flushed=None, layers_run: bool = True, stop: Optional[int] = None) -> Optional[torch.Tensor]:
        """Backward of _stack_fwd: bw["dx1"] holds the fp32 gradient of the final norm's output (nothing bypasses that norm); returns
        the fp32 gradient of the stack's input (x0, xb0).  The weight gradients of bw["group"] consecutive layers share a grouped
        launch; `flushed(i)` is called behind layer i when its launch has been queued.  Recompute mode: every layer's forward is issued
        again in front of its backward (_redo_layer).  LayerDrop: only the layers of _kept(stack) are walked (those the forward ran).
        Partial training (freeze.BackwardPlan.stack_walk): layers_run=False -- the final norm's own gradients only; stop = j -- the walk
        ends with the j-th kept layer, which computes no data gradient into its input.  Either way nothing is returned."""
        f, bw = self.flat, self.bw[stack]
        layers, D, H, pre, norm = self._stack(stack)
        acts = self._acts(stack)
        fm, fr = getattr(self, stack + "_fm"), getattr(self, stack + "_fr")
        # LayerDrop: the walk goes over the layers that ran.  Buffers, ring slots, the weight-gradient grouping, "the layer below" and
        # the bottom follow the position j in `kept`; parameters, dropout masks and the `flushed` report follow the index kept[j].
        kept = self._kept(stack)
        top, nbuf, group = len(kept) - 1, bw["nbuf"], bw["group"]
        Mo = M if sub is None else sub[2]                      # rows that left the stack
        grads = {} if self._skipped(norm) else dict(dgamma=f.gptr(norm + ".weight"), dbeta=f.gptr(norm + ".bias"))
        if not layers_run and top >= 0:
            # the floor is the final norm: its dgamma / dbeta only (the norm's input gradient goes to bw["dy"] and is not read)
            if pre:
                self._ln_pre_bwd(bw["dx1"], getattr(self, stack + "_sf"), f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["dy"], **grads)
            else:
                self._ln_bwd(bw["dx1"], acts[top].x2, f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["dy"], defer=False,
                             workspace=self.red_ws, **grads)
            return None
        if top < 0:
            # no layer ran: the final norm read the stack's input (its sub-rows), and its backward's output is the input's gradient
            x_in = x0 if sub is None else self.tail_x
            if pre:
                self._ln_pre_bwd(bw["dx1"], x_in, f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["dy"], **grads)
            else:
                self._ln_bwd(bw["dx1"], x_in, f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["dy"], defer=False,
                             workspace=self.red_ws, **grads)
            if sub is None:
                return bw["dy"]
            ops.unmask_rows_f32(bw["dy"], sub[1], bw["ds"], M=M, D=D, src_is_f32=True)      # back to all rows: zero where nothing went on
            return bw["ds"]
        if pre:
            # d(stream) for the top layer -- fp32 in bw["ds"], bf16 in its slot -- and that layer's linear2.bias gradient
            self._ln_pre_bwd(bw["dx1"], getattr(self, stack + "_sf"), f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["ds"],
                             ds_bf16=bw["dsb2"][top % nbuf], dbias=layers[kept[top]].gb2, **grads)
        else:
            self._ln_bwd(bw["dx1"], acts[top].x2, f.ptr32(norm + ".weight"), fm, fr, M=Mo, D=D, ds_f32=bw["dy"], defer=False,
                         workspace=self.red_ws, **grads)
        dy, dyb = bw["dy"], None
        last = 0 if stop is None else stop     # the lowest position whose backward runs
        for j in range(top, last - 1, -1):
            i = kept[j]
            w, a, sub_j = layers[i], acts[j], sub if j == top else None
            flush = (top - j) % group == group - 1 or j == last
            floor = stop is not None and j == stop
            if self.recompute:
                self._redo_layer(stack, j, x0, xb0, M, B, mask, seq, sub_j)
            if pre:
                # (the floor of a pre-norm stack still runs its own norm1 backward, for that norm's parameters; the stream gradient
                # it writes to bw["dy"] is not read, and the layer below gets nothing)
                dy, done = self._layer_bwd_pre(w, a, x0 if j == 0 else a.x1, layers[kept[j - 1]] if j > 0 and not floor else None, bw["dy"],
                                               M, D, H, B, mask, bw, j % nbuf, seq, sub=sub_j, flush=flush)
            else:
                x_in, xb_in = (x0, xb0) if j == 0 else (acts[j - 1].x2, acts[j - 1].x2b)
                dy, dyb, done = self._layer_bwd(w, a, x_in, xb_in, dy, dyb, bw["dy"], M, D, H, B, mask, bw, j % nbuf, seq, sub=sub_j,
                                                flush=flush, bottom=j == 0, stack=stack, li=i, **(dict(floor=True) if floor else {}))
            if done and flushed is not None:
                flushed(i)
        return None if stop is not None else dy

    # ------------------------------------------------------------------------------------------------ front-end
    def _frontend(self, audio: torch.Tensor) -> None:
        """audio bf16 [N, C_in, L] -> lf (fp32) / lf_b (bf16) [N*T, d_enc]   (reference jepa.py:391-396)"""
        c, f, C, S = self.cfg, self.flat, self.C, self.S
        self.front.forward(audio)
        M, T = self.M, self.T
        ops.layernorm_fwd(self.front.post_ptr[-1], f.ptr32("feature_norms.weight"), f.ptr32("feature_norms.bias"), M=M, D=C,
                          eps=c.norm_eps, y_bf16=self.fn_b, mean=self.fn_mean, rstd=self.fn_rstd, x_is_bf16=True,
                          in_seg=self.P[-1], in_valid=self.Tc, in_chan=S if S > 1 else 0)
        if self.has_mapper and self.fuse_add_pos and c.d_enc % 256 == 0 and C % 128 == 0:
            # mapper + positions in one launch (SURVEY K8 + K9): the position add rides in the GEMM's epilogue
            ops.gemm(self.fn_b, f.ptr16("post_extraction_mapper.weight"), self.lf_b, C2=self.lf, M=M, N=c.d_enc, K=C, lda=C, ldb=C,
                     ldc=c.d_enc, bias=f.ptr32("post_extraction_mapper.bias"), epilogue=ops.EPI_BF16_ADD_POS, aux=self.pos_enc, seg_rows=T)
            return
        if self.has_mapper:
            ops.gemm(self.fn_b, f.ptr16("post_extraction_mapper.weight"), self.map_b, M=M, N=c.d_enc, K=C, lda=C, ldb=C,
                     ldc=c.d_enc, bias=f.ptr32("post_extraction_mapper.bias"))
            src = self.map_b
        else:
            src = self.fn_b
        ops.add_pos(src, self.pos_enc, M=M, T=T, D=c.d_enc, y_f32=self.lf, y_bf16=self.lf_b)

    # ------------------------------------------------------------------------------------------------ backward
    def _backward_open(self, accumulate: bool = False, clear: bool = False) -> None:
        """What every step's backward starts with.  The flat gradient buffer is overwritten (accumulate=True: added to -- every
        parameter-gradient output of a backward adds into it, so the one difference is the clear here; clear=True: cleared whatever
        its state)."""
        self._folds = []                 # entries an exception in an earlier backward may have left behind must not be folded into this one
        f = self.flat
        if clear or (not accumulate and not f.g_clean):      # (FusedAdamW.fuse_zero_grad: the last update left the buffer clear)
            f.g32.zero_()
        f.g_clean = False
        self._accum_open = bool(accumulate)      # (set_frozen: the buffer holds sums made under the current frozen set)
        if self.deterministic:
            self._det_ws()              # (the slabs exist before the first launch; allocated once)
        self.refresh_wt()               # (a step that did it beside its forward: a no-op then)

    def _backward_close(self) -> None:
        self._flush_folds()
        self._join_side()                # all weight gradients are final before the optimiser / last all-reduce
        for bw in self.bw.values():
            bw["used"] = [False] * bw["nbuf"]

    def _frontend_bwd(self, dy: torch.Tensor, rag: bool = False, plan=None) -> None:
        """dy = d(local_features) fp32 [M, d_enc] -> gradients of the mapper, feature_norms and the conv stack.  rag: dy holds packed
        rows, those that `plan.inv` maps to their tokens (a JEPA step's context rows: zero on the others; the teacher branch is
        detached, jepa.py:408), and the conv backward may run over the plan's active rows only."""
        c, f = self.cfg, self.flat
        M, C, De = self.M, self.C, c.d_enc
        front, conv = not self._skipped("front"), not self._skipped("extract_audio")
        if not (front or conv):
            return
        if rag:
            ops.unmask_rows_f32(dy, plan.inv, self.d_lf_b, M=M, D=De, src_is_f32=True, dst_is_bf16=True)
            if not self.has_mapper:
                ops.unmask_rows_f32(dy, plan.inv, self.d_fn, M=M, D=De, src_is_f32=True)
                dy = self.d_fn
        else:
            ops.cast_f32_to_bf16(dy, self.d_lf_b, M * De)
        if self.has_mapper:
            if front:
                self._colsum_bf16(self.d_lf_b, f.gptr("post_extraction_mapper.bias"), M=M, N=De, ldx=De)
                self._wgrad(self.d_lf_b, self.fn_b, f.gptr("post_extraction_mapper.weight"), De, C, M)
            ops.gemm(self.d_lf_b, f.ptr16("post_extraction_mapper.weight"), self.d_fn, M=M, N=C, K=De, lda=De, ldb=C, ldc=C,
                     b_trans=1, epilogue=ops.EPI_ADD_F32)
            d_fn = self.d_fn
        else:
            d_fn = dy
        S, Tc = self.S, self.Tc
        # (a frozen conv stack: the backward stops here -- feature_norms' own gradients, no d(post[-1]); a frozen front above a
        # trainable conv stack: the data gradient only)
        grads = dict(dgamma=f.gptr("feature_norms.weight"), dbeta=f.gptr("feature_norms.bias")) if front else {}
        self._ln_bwd(d_fn, self.front.post_ptr[-1], f.ptr32("feature_norms.weight"), self.fn_mean, self.fn_rstd, M=M, D=C, defer=False,
                     ds_bf16=self.front.dpost_ptr[-1] if conv else None, **grads,
                     x_is_bf16=True, in_seg=self.P[-1], in_valid=Tc, out_seg=self.P[-1], out_valid=Tc, chan=S if S > 1 else 0)
        if not conv:
            return
        if self.grad_mult != 1.0:
            # feature_grad_mult (fairseq's GradMultiply on the conv output): one in-place pass over the bf16 d(post[-1]), rounded where
            # bf16 autocast rounds it; feature_norms and everything above saw the unscaled gradient.  (The C ABI has no scaling entry
            # for a bf16 tensor: this is torch's elementwise kernel.  Zero rows of a sparse step stay zero.)
            self.front.dpost[-1].mul_(self.grad_mult)
        # conv backward over the active rows only on a ragged step (sparse_conv), over every row otherwise
        self.front.backward(self, self.audio, plan if rag and self.sparse_conv else None)

    # ------------------------------------------------------------------------------------------------ inference
    def infer(self, audio: torch.Tensor, key_mask_u8: Optional[torch.Tensor]) -> torch.Tensor:
        """Student-only forward (reference jepa.py:456-467): returns fp32 [N, T, d_enc]."""
        c = self.cfg
        N = audio.shape[0]
        if N != self.N:
            self.alloc(N, train=False)
        self.wait_optimizer()
        self._drop_now = {}             # inference runs without dropout
        self._frontend(audio)
        self._stack_fwd("enc", self.lf, self.lf_b, self.M, N, key_mask_u8, y_f32=self.enc_out)
        return self.enc_out.view(N, self.T, c.d_enc)
