"""JEPA module for MI355X: the reference's LightningModule surface over the HIP engine.

Keeps the constructor, hooks, attributes, `ForwardReturn` keys and state_dict names/shapes of
reference wavjepa/jepa.py:24-467 (so reference checkpoints load and callers such as train.py / hear_api need no
change), but every tensor op of the step runs in `libwavjepa_hip.so` through `wavjepa_amd.engine`:
the nn.Modules below only hold parameters.  There is no PyTorch-op fallback; without the HIP library or a GPU the
compute entry points raise.
"""
from __future__ import annotations

import copy
import math
import os
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import ops
from .engine import EngineConfig, JepaEngine
from .extractors.audio_extractor import Extractor
from .freeze import check_grad_mult, is_student, match
from .functions import trunc_normal_
from .layerdrop import check_keep, check_rate, kept_layers
from .mask_plan import MaskPlan, make_mask_plan
from .optim import MAX_GROUPS, resolve_groups, trainable
from .params import FlatParams
from .pos_embed import get_1d_sincos_pos_embed_from_grid
from .types import ForwardReturn, TransformerEncoderCFG, TransformerLayerCFG, activation_kind_of
from .upload import pack_upload


def collate_fn(batch: torch.Tensor) -> torch.Tensor:
    return batch.flatten(start_dim=0, end_dim=1)


class _AttrDict(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


# ---------------------------------------------------------------------------------------------------------------------
# Parameter containers with nn.TransformerEncoder's state_dict names (…layers.{i}.self_attn.in_proj_weight, …)
# ---------------------------------------------------------------------------------------------------------------------
class _SelfAttention(nn.Module):
    def __init__(self, d: int, bias: bool = True):
        super().__init__()
        self.in_proj_weight = nn.Parameter(torch.empty(3 * d, d))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d))
        self.out_proj = nn.Linear(d, d, bias=bias)
        nn.init.xavier_uniform_(self.in_proj_weight)          # nn.MultiheadAttention._reset_parameters
        nn.init.constant_(self.out_proj.bias, 0.0)


class _PostNormLayer(nn.Module):
    def __init__(self, d_model: int, nhead: int, dim_feedforward: int, layer_norm_eps: float, **unused):     # (dropout: TransformerStack.dropout)
        super().__init__()
        self.self_attn = _SelfAttention(d_model)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.nhead = nhead


class _PreNormLayer(_PostNormLayer):
    """The same parameters, names and initialisation; the engine runs x = x + branch(norm(x)) (nn.TransformerEncoderLayer norm_first=True)."""
    norm_first = True


class TransformerStack(nn.Module):
    """`num_layers` deep copies of one layer (post-norm, or pre-norm with norm_first=True) + final LayerNorm (as
    nn.TransformerEncoder(layer, norm=...)).  Both layouts have the same parameter names and shapes."""

    def __init__(self, layer_cfg: Dict[str, Any], num_layers: int):
        super().__init__()
        self.norm_first = bool(layer_cfg.get("norm_first", False))
        # the feed-forward activation's kind: it runs in linear1's GEMM epilogue (engine._mlp_fwd), the module itself is never called
        self.activation = activation_kind_of(layer_cfg.get("activation"))
        # dropout: the rate of this stack's layers in a training-mode forward (engine: the _drop kernels; 0 = the launches without it)
        self.dropout = float(layer_cfg.get("dropout", 0.0) or 0.0)
        if not (0.0 <= self.dropout < 1.0):
            raise ValueError(f"dropout must lie in [0, 1), not {layer_cfg.get('dropout')}")
        if self.dropout > 0 and self.norm_first:
            raise NotImplementedError(f"dropout={self.dropout} with norm_first=True: the dropout kernels cover post-norm layers only")
        if self.dropout > 0 and int(layer_cfg["d_model"]) // int(layer_cfg["nhead"]) not in (32, 64):
            raise NotImplementedError(f"dropout={self.dropout} with {int(layer_cfg['d_model']) // int(layer_cfg['nhead'])}-wide heads "
                                      f"(d_model={layer_cfg['d_model']}, nhead={layer_cfg['nhead']}): attention dropout runs in the "
                                      "streamed kernels, which take head widths 32 and 64")
        if int(layer_cfg["dim_feedforward"]) != 4 * int(layer_cfg["d_model"]):
            raise NotImplementedError("feed-forward width must be 4 * d_model")
        first = (_PreNormLayer if self.norm_first else _PostNormLayer)(**layer_cfg)
        self.layers = nn.ModuleList([first] + [copy.deepcopy(first) for _ in range(num_layers - 1)])
        self.norm = nn.LayerNorm(layer_cfg["d_model"])
        self.d_model, self.nhead, self.num_layers = int(layer_cfg["d_model"]), int(layer_cfg["nhead"]), num_layers
        self.layer_norm_eps = float(layer_cfg["layer_norm_eps"])


# ---------------------------------------------------------------------------------------------------------------------
# Autograd bridge: loss.backward() runs the engine's hand-written backward into the flat gradient buffer
# ---------------------------------------------------------------------------------------------------------------------
class _StepOutputs(dict):
    """The reference's ForwardReturn (a plain dict).  `preds` in the reference's dense [N*G, T, D] shape is materialised
    on first access: the training loop never reads it, and on a ragged step the engine holds only the visible rows
    (the others, which carry zero loss weight at reference jepa.py:356, read 0)."""

    def __init__(self, engine, **items):
        super().__init__(**items)
        self._engine, self._plan = engine, engine.plan

    def __missing__(self, key):
        if key != "preds":
            raise KeyError(key)
        if self._engine.plan is not self._plan:
            raise RuntimeError("preds belongs to an earlier step: read it before the next forward overwrites the arena")
        value = self._engine.dense_preds()
        self[key] = value
        return value

    def __contains__(self, key):
        return key == "preds" or super().__contains__(key)

    def get(self, key, default=None):
        return self[key] if key in self else default


class _EngineLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor: torch.Tensor, module: "JEPA") -> torch.Tensor:
        ctx.module = module
        return module._engine.loss[0].clone()

    @staticmethod
    def backward(ctx, grad_out: torch.Tensor):
        m = ctx.module
        g = grad_out.contiguous().float()
        if m.accumulate_grads:           # torch's contract: backward adds, FusedAdamW.zero_grad() clears
            m._engine.backward(gscale_ptr=g.data_ptr(), on_grads_ready=m._grads_ready_hook, accumulate=True)
        else:
            m._engine.backward(gscale_ptr=g.data_ptr(), on_grads_ready=m._grads_ready_hook)
        m._flat.attach_grads()
        return torch.zeros_like(m._anchor), None


_ADAMW_SIDE = os.environ.get("WJ_ADAMW_SIDE", "1") != "0"
# workgroups of the overlapped update: one per CU -- it should take the HBM the front-end kernels leave idle, not their CU slots
# (a full grid of 8192: 45.68 ms/step, 1024: 45.64, 512: 45.48, 256: 45.40, interleaved on one box; 128 / 192 / 384 within 0.1 of 256)
_ADAMW_SIDE_WGS = int(os.environ.get("WJ_ADAMW_SIDE_WGS", "256"))
_ADAMW_ZERO_GRAD = os.environ.get("WJ_ADAMW_ZERO_GRAD", "1") != "0"


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics (reference jepa.py:215-222) as ONE kernel over the flat parameter buffer, with the
    global-norm clip of Lightning's gradient_clip_val (train.py:177-178) fused in (`max_grad_norm`).

    groups (wavjepa_amd.optim): None -- one group of every trainable parameter, the reference's configure_optimizers, updated by
    wj_adamw_step; or a list of {"params": [names or Parameters], "lr": ..., "weight_decay": ...} (both default to the constructor's)
    that puts every trainable parameter into exactly one group, at most 64 of them.  The update is then wj_adamw_groups_step: still
    one pass over the flat buffers, the group of an element looked up in a byte map (FlatParams.group_map).  step() reads lr and
    weight_decay of EVERY group from self.param_groups at each call, so LambdaLR and a user's weight-decay schedule both apply;
    betas, eps and the clip (one global norm) are common to all groups."""

    def __init__(self, module: "JEPA", lr: float, betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.01,
                 max_grad_norm: float = 0.0, groups=None):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self._assignment = None          # {parameter name: group index} of a grouped optimiser
        self._group_map = None           # its device byte map, made with the flat buffers
        if groups is None:
            params = [p for _, p in trainable(module)]
        else:
            params, self._assignment = resolve_groups(module, groups, defaults)
        super().__init__(params, defaults)
        self._module = module
        # Partial training: the parameters the module holds frozen (JEPA.freeze, requires_grad_(False), feature_grad_mult = 0, the
        # freeze_feature_extractor_updates schedule) move into ONE extra group with lr = 0 and weight_decay = 0 -- p - 0 * x is p
        # exactly, in the fp32 master and its bf16 shadow -- which exists only while something is frozen; step() reads the set again
        # at every call.  _home: every group's full parameter list, to which a released parameter returns.
        self._home = [list(q["params"]) for q in self.param_groups]
        self._names = {id(p): n for n, p in trainable(module)}
        self._frozen_seen: frozenset = frozenset()
        self._frozen_assignment = None
        self._map_memo: Dict[frozenset, torch.Tensor] = {}       # frozen set -> its device byte map (a few: a schedule has two)
        self._sync_frozen_group()
        self.max_grad_norm = max_grad_norm
        self._t = 0
        self._sumsq = None
        self._ws = None
        # overlap_next_forward (set by the training loop, trainer.StepRunner; WJ_ADAMW_SIDE=0 keeps it off): only the conv extractor, the
        # feature norm and the post-extraction mapper are updated on the compute stream; the transformer stacks (99 % of the parameters,
        # ~0.65 ms of streaming) go to the engine's side stream, where they run beside the NEXT step's crop / conv0 / conv stack -- matrix-
        # and VALU-bound kernels that leave the HBM idle, on a side stream that has nothing to do until the conv features exist.  The
        # engine's forward waits for the event before its first transformer kernel (JepaEngine.wait_optimizer); so do state_dict, the EMA
        # and inference.  Off by default: a caller that reads parameters right behind step() on its own stream would race the update.
        # With it on, readers that do NOT go through the engine -- a submodule's state_dict (model.encoder.state_dict()), copy.deepcopy,
        # direct p.data reads -- must call model._engine.wait_optimizer() first; JEPA.state_dict / load_state_dict / _apply (.cpu(), .to())
        # and Trainer.fit's return do so themselves.
        self.overlap_next_forward = False
        # fuse_zero_grad (training loop only; WJ_ADAMW_ZERO_GRAD=0 keeps it off): the update clears the gradient it has just read
        # (wj_adamw_args.zero_grad), so the next backward starts from a clean flat buffer without its own 444-MB fill on the critical path.
        # p.grad then reads 0 after step() -- what zero_grad() leaves; a caller that inspects gradients after step() keeps it off.
        self.fuse_zero_grad = False

    def _sync_frozen_group(self) -> None:
        """Follow the module's frozen set: the lr = 0 group holds exactly the frozen parameters (and is absent when there are none),
        every other group what is left of its own."""
        names_of = getattr(self._module, "_frozen_for_update", None)
        frozen = names_of() if names_of is not None else frozenset()
        if frozen == self._frozen_seen:
            return
        base = [q for q in self.param_groups if not q.get("frozen")]
        if frozen and len(base) + 1 > MAX_GROUPS:
            raise ValueError(f"{len(base)} parameter groups and the group of frozen parameters: FusedAdamW takes at most {MAX_GROUPS}")
        for q, home in zip(base, self._home):
            q["params"] = [p for p in home if self._names[id(p)] not in frozen]
        self.param_groups[:] = base
        self._frozen_assignment = None
        if frozen:
            held = [p for home in self._home for p in home if self._names[id(p)] in frozen]
            self.param_groups.append(dict(self.defaults, params=held, lr=0.0, weight_decay=0.0, frozen=True))
            own = self._assignment or {}
            self._frozen_assignment = {n: (len(base) if n in frozen else own.get(n, 0)) for n in self._names.values()}
        self._frozen_seen = frozen
        self._group_map = self._map_memo.get(frozen)         # (the byte map of a set seen before, while the flat buffers are the same)

    def _ensure_scratch(self, flat) -> None:
        if self._sumsq is None:
            self._sumsq = torch.zeros(1, dtype=torch.float32, device=flat.device)
            self._ws = torch.empty(1024, dtype=torch.float32, device=flat.device)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:          # Lightning's automatic optimisation hands training_step + backward over as a closure
            with torch.enable_grad():
                loss = closure()
        m = self._module
        m._ensure_engine()
        flat = m._flat
        flat.ensure_adam_state()
        self._ensure_scratch(flat)
        self._sync_frozen_group()
        g = self.param_groups[0]
        self._t += 1
        if self.max_grad_norm > 0:
            ops.grad_sumsq(flat.g32, self._sumsq, self._ws, flat.n)
        zg = bool(self.fuse_zero_grad) and _ADAMW_ZERO_GRAD
        kw = dict(beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], step=self._t,
                  max_norm=self.max_grad_norm, sumsq=self._sumsq if self.max_grad_norm > 0 else None)
        assignment = self._frozen_assignment or self._assignment      # (with something frozen: the groups and the lr = 0 group behind them)
        if assignment is None:
            kw.update(lr=float(g["lr"]), weight_decay=g["weight_decay"])
            adamw = ops.adamw_step
        else:                            # every group's pair, read now: schedulers and the user write them between steps
            if self._group_map is None or self._group_map.device != flat.p32.device or self._group_map.numel() * 8 != flat.n:
                self._group_map = flat.group_map(assignment)
                if self._frozen_assignment is not None:
                    if len(self._map_memo) >= 4:
                        self._map_memo.clear()
                    self._map_memo[self._frozen_seen] = self._group_map
            live = lambda q, key: 0.0 if q.get("frozen") else float(q[key])      # (whatever a scheduler wrote into the frozen group)
            kw.update(lr=[live(q, "lr") for q in self.param_groups], weight_decay=[live(q, "weight_decay") for q in self.param_groups],
                      group_map=self._group_map)
            adamw = ops.adamw_groups_step

        def update(lo: int, hi: int, workgroups: int = 0) -> None:
            where = {} if assignment is None else dict(first=lo)
            adamw(flat.p32.data_ptr() + 4 * lo, flat.g32.data_ptr() + 4 * lo, flat.adam_m.data_ptr() + 4 * lo,
                  flat.adam_v.data_ptr() + 4 * lo, hi - lo, p_bf16=flat.p16.data_ptr() + 2 * lo, workgroups=workgroups, zero_grad=zg, **where, **kw)
        eng = m._engine
        front, rest = flat.front_and_rest_ranges()
        if self.overlap_next_forward and eng.use_side and rest and _ADAMW_SIDE:
            for lo, hi in front:
                update(lo, hi)
            eng.optimizer_on_side(lambda: [update(lo, hi, _ADAMW_SIDE_WGS) for lo, hi in rest])
        else:
            update(0, flat.n)
        flat.g_clean = zg            # engine.backward skips its own clear of the flat gradient buffer
        m._student_bf16_fresh = True
        return loss

    def grad_norm(self) -> torch.Tensor:
        """Global L2 norm of the last step's gradients (device scalar; no sync)."""
        return self._sumsq.sqrt() if self._sumsq is not None else torch.zeros(1)

    def zero_grad(self, set_to_none: bool = True) -> None:  # the engine overwrites the flat gradient buffer each backward
        m = self._module
        if not m.accumulate_grads or m._flat is None or m._engine is None:
            return None
        # JEPA.accumulate_grads: backward adds into the flat buffer, so this call is the clear (the views stay attached whatever
        # set_to_none says: the buffer IS the gradients).  Nothing to do behind an update that cleared it itself (fuse_zero_grad).
        if not m._flat.g_clean:
            m._engine.wait_optimizer()       # an update overlapped on the side stream may still read the buffer
            m._flat.g32.zero_()
            m._flat.g_clean = True
        return None

    def state_dict(self):
        flat = self._module._flat
        if self._module._engine is not None:
            self._module._engine.wait_optimizer()
        sd = dict(step=self._t, lr=self.param_groups[0]["lr"], m=None if flat is None or flat.adam_m is None else flat.adam_m.cpu(),
                  v=None if flat is None or flat.adam_v is None else flat.adam_v.cpu())
        if self._assignment is not None:     # a grouped optimiser: every group's pair, for the reason given for lr below
            own = [q for q in self.param_groups if not q.get("frozen")]      # (the lr = 0 group of frozen parameters follows the module)
            sd["group_lr"] = [float(q["lr"]) for q in own]
            sd["group_weight_decay"] = [float(q["weight_decay"]) for q in own]
        return sd

    def load_state_dict(self, sd):
        self._t = int(sd["step"])
        if sd.get("lr") is not None:     # LambdaLR.load_state_dict does not write the group lr back: without this the first
            self.param_groups[0]["lr"] = float(sd["lr"])   # resumed step would run at the constructor's lr
        if self._assignment is not None and sd.get("group_lr") is not None:
            own = [q for q in self.param_groups if not q.get("frozen")]
            if len(sd["group_lr"]) != len(own) or len(sd["group_weight_decay"]) != len(own):
                raise ValueError(f"the optimiser state holds {len(sd['group_lr'])} parameter groups, this optimiser has {len(own)}")
            for q, lr, wd in zip(own, sd["group_lr"], sd["group_weight_decay"]):
                q["lr"], q["weight_decay"] = float(lr), float(wd)
        self._module._ensure_engine().wait_optimizer()
        flat = self._module._flat
        flat.ensure_adam_state()
        if sd.get("m") is not None:
            flat.adam_m.copy_(sd["m"])
            flat.adam_v.copy_(sd["v"])


def cosine_schedule_with_warmup(optimizer, num_warmup_steps: int, num_training_steps: int):
    """HF get_cosine_schedule_with_warmup (num_cycles=0.5), which the reference calls at jepa.py:224-225."""
    def lr_lambda(step: int) -> float:
        if step < num_warmup_steps:
            return float(step) / float(max(1, num_warmup_steps))
        progress = float(step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))

    return _GroupLambdaLR(optimizer, lr_lambda)


class _GroupLambdaLR(torch.optim.lr_scheduler.LambdaLR):
    """LambdaLR over the groups the optimiser has NOW: FusedAdamW's lr = 0 group of frozen parameters comes and goes with the frozen set
    (LambdaLR itself pairs the groups with the learning rates of the groups it was built with).  That group keeps lr 0; every other
    group gets initial_lr * lambda(step), LambdaLR's own value."""

    def get_lr(self):
        factor = self.lr_lambdas[0](self.last_epoch)
        return [0.0 if g.get("frozen") else g["initial_lr"] * factor for g in self.optimizer.param_groups]


def accumulate_window(module) -> int:
    """k = accumulate_grad_batches of the trainer `module` is attached to (Lightning's attribute name); 1 where there is none."""
    try:
        k = getattr(module.trainer, "accumulate_grad_batches", 1)
    except (RuntimeError, AttributeError):       # Lightning: not attached to a Trainer yet
        k = 1
    return 1 if k is None else int(k)


def dropout_call_of(global_step: int, k: int = 1, micro: int = 0, explicit: Optional[int] = None) -> int:
    """The dropout generator's call counter of a training forward: an explicit model.dropout_call, else global_step * k + micro for
    micro-batch `micro` of a window of k (k = 1: global_step), so that the micro-batches of one optimiser step draw different masks.
    The counter is 32 bits wide in the kernels (wj_dropout_args.call): a product beyond that would wrap onto an earlier step's masks."""
    if explicit is not None:
        return int(explicit)
    if k == 1:
        return int(global_step)
    if not 0 <= micro < k:
        raise ValueError(f"micro-batch index {micro} outside a window of {k}")
    call = int(global_step) * int(k) + int(micro)
    if call >= 1 << 32:
        raise OverflowError(f"dropout call counter global_step * accumulate_grad_batches + micro = {global_step} * {k} + {micro} does not "
                            "fit the generator's 32-bit counter")
    return call


class _NullTrainer:
    max_steps = 375000


# The reference's JEPA is a pytorch_lightning.LightningModule (reference jepa.py:24).  When Lightning is importable this class
# derives from it too, so pl.Trainer.fit(model, datamodule) accepts it (hooks: on_after_batch_transfer, training_step,
# configure_optimizers; `hparams` through save_hyperparameters; `global_step` / `trainer` / `device` / `log_dict` are Lightning's
# own).  Without Lightning (this image ships none) it is a plain nn.Module that provides those attributes itself and
# wavjepa_amd.trainer.Trainer drives it.
try:                                         # pragma: no cover - depends on the environment
    import pytorch_lightning as _pl
except Exception:                            # noqa: BLE001
    try:
        import lightning.pytorch as _pl
    except Exception:                        # noqa: BLE001
        _pl = None
HAS_LIGHTNING = _pl is not None
_ModuleBase = _pl.LightningModule if HAS_LIGHTNING else nn.Module


def loss_kind_of(loss_fn: Optional[nn.Module]) -> Tuple[str, float]:
    """(kind, beta) of the masked objective the reference would compute with `loss_fn` (jepa.py:351: loss_fn(pred, target) per element,
    so reduction must be 'none').  None / MSELoss -> mse; L1Loss -> l1; SmoothL1Loss(beta) -> smooth_l1 (beta = 0 is L1, as torch defines
    it); HuberLoss(delta) -> huber.  Anything else is refused here instead of being trained as MSE."""
    if loss_fn is None:
        return "mse", 1.0
    table = ((nn.MSELoss, "mse", None), (nn.SmoothL1Loss, "smooth_l1", "beta"), (nn.HuberLoss, "huber", "delta"), (nn.L1Loss, "l1", None))
    for cls, kind, attr in table:
        if type(loss_fn) is cls:
            break
    else:
        raise NotImplementedError(f"loss_fn {type(loss_fn).__name__}: the loss kernel computes nn.MSELoss, nn.L1Loss, nn.SmoothL1Loss "
                                  "and nn.HuberLoss")
    if getattr(loss_fn, "reduction", "none") != "none":
        raise ValueError(f"loss_fn must be built with reduction='none' (got {loss_fn.reduction!r}): the masked mean over target rows "
                         "is taken by the loss kernel")
    beta = 1.0 if attr is None else float(getattr(loss_fn, attr))
    if kind == "smooth_l1" and beta == 0.0:
        return "l1", 1.0
    if attr is not None and not (beta > 0.0 and beta < float("inf")):
        raise ValueError(f"loss_fn {type(loss_fn).__name__}: {attr} must be positive and finite (got {beta})")
    return kind, beta


class JEPA(_ModuleBase):
    """Joint-Embedding Predictive Architecture for waveforms (student encoder + predictor vs EMA teacher)."""
    student_layout = True        # FlatParams / the optimiser hold every student parameter, frozen or not (freeze.is_student)

    def __init__(self, feature_extractor: Extractor, transformer_encoder_layers_cfg: TransformerLayerCFG,
                 transformer_encoder_cfg: TransformerEncoderCFG, transformer_decoder_layers_cfg: TransformerLayerCFG,
                 transformer_decoder_cfg: TransformerEncoderCFG, decoder_embedding_dim: int = 512, loss_fn: Optional[nn.Module] = None,
                 lr: float = 0.0002, adam_betas=(0.9, 0.98), adam_eps: float = 1e-06, adam_weight_decay: float = 0.01,
                 ema_decay: float = 0.999, ema_end_decay: float = 0.99999, ema_anneal_end_step: int = 100000,
                 average_top_k_layers: int = 12, resample_sr: int = 16000, process_audio_seconds: float = 2.00,
                 nr_samples_per_audio: int = 16, use_gradient_checkpointing: bool = False, compile_modules: bool = False,
                 size: str = "base", warmup_steps: int = 100000, **kwargs: Any):
        super().__init__()
        self.sr = resample_sr
        self.nr_samples_per_audio = nr_samples_per_audio
        self.ema_end_step = ema_anneal_end_step
        self.target_length = int(resample_sr * process_audio_seconds)
        self.total_patches = feature_extractor.total_patches(self.target_length)
        self.use_compiled_forward = False            # there is no tracing compiler on this path: kernels are hand-written
        # activation recomputation in the engine (EngineConfig.recompute): the student AND the predictor keep one output per layer and
        # compute the rest again in the backward, with the masks of the first pass (the reference checkpoints the student only, and
        # its call drops the key mask: jepa.py:449-450)
        self.use_gradient_checkpointing = bool(use_gradient_checkpointing)
        if HAS_LIGHTNING:        # as the reference does (jepa.py:105-107): hyper-parameters into the checkpoint
            self.save_hyperparameters(ignore=["feature_encoder", "feature_extractor", "loss_fn"])
            self.hparams["adam_betas"] = tuple(adam_betas)
            self.hparams.pop("weight_decay_exclude", None)     # (recorded below, only when set)
            self.hparams.pop("layer_lr_decay", None)
            self.hparams.pop("encoder_layerdrop", None)
            self.hparams.pop("decoder_layerdrop", None)
            self.hparams.pop("feature_grad_mult", None)
            self.hparams.pop("freeze_feature_extractor_updates", None)
        else:
            self.hparams = _AttrDict(lr=lr, adam_betas=tuple(adam_betas), adam_eps=adam_eps, adam_weight_decay=adam_weight_decay,
                                     ema_decay=ema_decay, ema_end_decay=ema_end_decay, ema_anneal_end_step=ema_anneal_end_step,
                                     average_top_k_layers=average_top_k_layers, resample_sr=resample_sr,
                                     process_audio_seconds=process_audio_seconds, nr_samples_per_audio=nr_samples_per_audio,
                                     compile_modules=compile_modules, size=size, warmup_steps=warmup_steps,
                                     decoder_embedding_dim=decoder_embedding_dim)
            if self.use_gradient_checkpointing:      # recorded only when set, the rule of norm_first_encoder below
                self.hparams["use_gradient_checkpointing"] = True
            self.global_step = 0
            self.trainer = _NullTrainer()
        # Parameter groups of the optimiser (wavjepa_amd.optim.param_groups): which parameters go without weight decay (None, "1d" or
        # fnmatch patterns on names) and BEiT's layer-wise lr decay.  Recorded only when set, the rule of norm_first_encoder below:
        # a default model keeps its hyper-parameter set and the single group of the reference's configure_optimizers.
        # Both are keywords taken through **kwargs (weight_decay_exclude=None, layer_lr_decay=1.0): the named parameters stay the reference's.
        weight_decay_exclude, layer_lr_decay = kwargs.pop("weight_decay_exclude", None), kwargs.pop("layer_lr_decay", 1.0)
        if weight_decay_exclude is not None and not isinstance(weight_decay_exclude, str):
            weight_decay_exclude = tuple(weight_decay_exclude)
        self.weight_decay_exclude, self.layer_lr_decay = weight_decay_exclude, float(layer_lr_decay)
        if self.weight_decay_exclude is not None:
            self.hparams["weight_decay_exclude"] = self.weight_decay_exclude
        if self.layer_lr_decay != 1.0:
            self.hparams["layer_lr_decay"] = self.layer_lr_decay
        # LayerDrop (wavjepa_amd.layerdrop; fairseq's TransformerEncoder, no rescaling): in a training-mode forward every layer of the
        # student / the predictor is skipped for the whole batch with this probability -- no launch, the stream passes unchanged, the
        # layer's gradient is the zero of the cleared buffer (the fused AdamW sees that zero: INTEGRATION.md, differences by design).
        # The teacher, eval mode and inference never drop.  Keywords through **kwargs as well (encoder_layerdrop=0.0,
        # decoder_layerdrop=0.0), each recorded only when set.
        self.encoder_layerdrop = check_rate(kwargs.pop("encoder_layerdrop", 0.0), "encoder_layerdrop")
        self.decoder_layerdrop = check_rate(kwargs.pop("decoder_layerdrop", 0.0), "decoder_layerdrop")
        if self.encoder_layerdrop > 0:
            self.hparams["encoder_layerdrop"] = self.encoder_layerdrop
        if self.decoder_layerdrop > 0:
            self.hparams["decoder_layerdrop"] = self.decoder_layerdrop
        # Partial training (wavjepa_amd.freeze).  A student parameter with requires_grad=False -- by freeze(), or by hand -- is not trained:
        # no gradient, no update, no weight decay; its unit's parameter-gradient launches are not issued and the backward ends at the
        # lowest trainable unit.  feature_grad_mult (fairseq's GradMultiply on the conv output, in [0, 1]): the factor on the gradient
        # that enters the conv stack; 0 freezes extract_audio.*.  freeze_feature_extractor_updates = n: extract_audio.* is frozen while
        # global_step < n.  Keywords through **kwargs (feature_grad_mult=1.0, freeze_feature_extractor_updates=0), each recorded only when set.
        self.feature_grad_mult = check_grad_mult(kwargs.pop("feature_grad_mult", 1.0))
        self.freeze_feature_extractor_updates = int(kwargs.pop("freeze_feature_extractor_updates", 0) or 0)
        if self.freeze_feature_extractor_updates < 0:
            raise ValueError(f"freeze_feature_extractor_updates={self.freeze_feature_extractor_updates} must not be negative")
        if self.feature_grad_mult != 1.0:
            self.hparams["feature_grad_mult"] = self.feature_grad_mult
        if self.freeze_feature_extractor_updates > 0:
            self.hparams["freeze_feature_extractor_updates"] = self.freeze_feature_extractor_updates
        self._student_named: Optional[List[Tuple[str, nn.Parameter]]] = None     # cached (name, Parameter) of the student, layout order
        self._frozen_key, self._frozen_set = None, frozenset()
        self._frozen_memo: Dict[tuple, frozenset] = {}
        self._frozen_step: Optional[frozenset] = None          # the frozen set of the last training forward (the optimiser's)
        # layerdrop_keep: None -- the kept layers are drawn per forward from (dropout_seed, the dropout call counter, stack, layer), the
        # same on every data-parallel rank; {"enc": [...], "dec": [...]} fixes the kept set of the stacks it names (sorted distinct
        # layer indices; an empty list is legal) for every training forward until it is reset.  last_kept: the kept lists of the last
        # training forward that ran under LayerDrop (None before the first).
        self._layerdrop_keep: Optional[Dict[str, List[int]]] = None
        self.last_kept: Optional[Dict[str, List[int]]] = None
        self.extract_audio = feature_extractor
        self.feature_norms = nn.LayerNorm(self.extract_audio.embedding_dim)
        self.loss_fn = loss_fn
        # the module is not called: its kind runs inside the loss kernel (ops.masked_loss).  Recorded only when it is not MSE, so that
        # checkpoints of MSE models keep the hyper-parameter set they always had
        self.loss_kind, self.loss_beta = loss_kind_of(loss_fn)
        if self.loss_kind != "mse":
            self.hparams["loss"] = self.loss_kind
            self.hparams["loss_beta"] = self.loss_beta

        enc_l, enc_c = dict(transformer_encoder_layers_cfg), dict(transformer_encoder_cfg)
        dec_l, dec_c = dict(transformer_decoder_layers_cfg), dict(transformer_decoder_cfg)
        if size == "large":    # ViT-Large student (reference jepa.py:114-118)
            enc_l.update(nhead=16, d_model=1024, dim_feedforward=4096)
            enc_c.update(num_layers=24)
        elif size == "tiny":
            # BASELINE config 1 (a build-defined size, the reference knows base / large only): 2-layer student d = 128,
            # 2-layer predictor d = 64 with 4 heads (head dim 16: wj_attn_* run it in their 32-wide geometry).
            enc_l.update(nhead=4, d_model=128, dim_feedforward=512)
            enc_c.update(num_layers=2)
            dec_l.update(nhead=4, d_model=64, dim_feedforward=256)
            dec_c.update(num_layers=2)
            self.hparams["average_top_k_layers"] = min(int(average_top_k_layers), 2)
        self.n_encoder_heads = enc_l["nhead"]
        self.encoder_embedding_dim = enc_l["d_model"]
        self.n_decoder_heads = dec_l["nhead"]
        self.decoder_embedding_dim = dec_l["d_model"]          # the ctor's decoder_embedding_dim is ignored upstream too

        self.encoder = TransformerStack(enc_l, enc_c["num_layers"])
        c_feat = feature_extractor.embedding_dim
        self.post_extraction_mapper = nn.Linear(c_feat, self.encoder_embedding_dim) if c_feat != self.encoder_embedding_dim else None
        self.decoder = TransformerStack(dec_l, dec_c["num_layers"])
        # recorded only when set: checkpoints of post-norm models keep the hyper-parameter set they always had
        if self.encoder.norm_first:
            self.hparams["norm_first_encoder"] = True
        if self.decoder.norm_first:
            self.hparams["norm_first_decoder"] = True
        # the feed-forward activation of the student (and so of its EMA teacher) and of the predictor: the same rule
        if self.encoder.activation != "gelu":
            self.hparams["activation_encoder"] = self.encoder.activation
        if self.decoder.activation != "gelu":
            self.hparams["activation_decoder"] = self.decoder.activation
        # Dropout in the student and the predictor of a training-mode forward; the TEACHER runs without it (differences
        # by design).  The masks are a function of (dropout_seed, dropout_call or global_step, stack, layer, site, element): nothing is
        # stored, a resumed run continues the same mask sequence.  Recorded only when some rate is set (the rule of norm_first_*).
        self._dropout_seed = int(torch.initial_seed())
        self.dropout_call: Optional[int] = None       # None: int(global_step) (under accumulation: dropout_call_of)
        if self.encoder.dropout > 0 or self.decoder.dropout > 0:
            self.hparams["dropout_encoder"] = self.encoder.dropout
            self.hparams["dropout_decoder"] = self.decoder.dropout
            self.hparams["dropout_seed"] = self._dropout_seed
        elif self.encoder_layerdrop > 0 or self.decoder_layerdrop > 0:     # LayerDrop draws from the same seed and counter
            self.hparams["dropout_seed"] = self._dropout_seed
        # Collapse monitor (an attribute, no constructor argument: signature and hyper-parameters are what they were).  A training-mode
        # forward at a step with global_step % monitor_every == 0 returns pred_var / target_var (device scalars: the mean over
        # features of sqrt(variance over the loss's rows + 1e-6)) and training_step logs them; 0 = never, the step as it always was.
        self.monitor_every: int = 0
        # Gradient accumulation (attributes as well).  accumulate_grads: loss.backward() ADDS into the flat gradient buffer and
        # FusedAdamW.zero_grad() clears it -- torch's contract, what a loop of k backwards per optimiser step needs; off, every backward
        # starts from a clear buffer and zero_grad() is a no-op, as always.  _micro = (i, k): the micro-batch index inside a window of
        # trainer.accumulate_grad_batches = k, set by training_step for the forward it issues ((0, 1) anywhere else).
        self.accumulate_grads: bool = False
        self._micro: Tuple[int, int] = (0, 1)
        self.decoder_to_encoder_mapper = nn.Linear(self.decoder_embedding_dim, self.encoder_embedding_dim, bias=True)
        self.encoder_to_decoder_mapper = nn.Linear(self.encoder_embedding_dim, self.decoder_embedding_dim)
        self.mask_token = nn.Parameter(torch.zeros(1, 1, self.decoder_embedding_dim))
        nn.init.normal_(self.mask_token, std=0.02)
        self.pos_encoding_encoder = self._get_pos_embed_params(self.encoder_embedding_dim)
        self.pos_encoding_decoder = self._get_pos_embed_params(self.decoder_embedding_dim)
        self.apply(self._init_weights)
        self._init_teacher()
        self.collate_fn = collate_fn

        self._flat: Optional[FlatParams] = None
        self._engine: Optional[JepaEngine] = None
        self._anchor: Optional[torch.Tensor] = None
        self._student_bf16_fresh = False
        self._teacher_bf16_fresh = False
        self._grads_ready_hook = None
        self._adam_carry = None
        self._logged: Dict[str, Any] = {}

    # ------------------------------------------------------------------------------------------------ construction
    def _init_weights(self, m: nn.Module) -> None:
        if isinstance(m, nn.Linear):
            trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def _get_pos_embed_params(self, embedding_dim: int) -> nn.Parameter:
        tab = get_1d_sincos_pos_embed_from_grid(embedding_dim, np.arange(self.total_patches, dtype=np.float64))
        return nn.Parameter(torch.from_numpy(tab).float().unsqueeze(0), requires_grad=False)

    def _init_teacher(self) -> None:
        self.teacher_encoder = copy.deepcopy(self.encoder)
        self.teacher_encoder.requires_grad_(False)

    # ------------------------------------------------------------------------------------------------ device / engine
    if not HAS_LIGHTNING:        # Lightning provides `device`, `log_dict`, `global_step` and `trainer` itself
        @property
        def device(self) -> torch.device:
            return self.mask_token.device

        def log_dict(self, data: Dict[str, Any], **kw) -> None:
            self._logged = dict(data)
            log = getattr(self.trainer, "log_dict", None)
            if log is not None:
                log(data, **kw)

    def _max_steps(self) -> int:
        try:
            steps = int(self.trainer.max_steps)
        except (RuntimeError, AttributeError, TypeError):      # Lightning: not attached to a Trainer yet
            steps = -1
        return steps if steps > 0 else _NullTrainer.max_steps

    def _apply(self, fn, *a, **k):
        if getattr(self, "_engine", None) is not None:
            # .cpu() / .to() / .half() read every parameter (and the moments carried below): an update overlapped with the next forward
            # (FusedAdamW.overlap_next_forward) may still be writing them on the engine's side stream
            self._engine.wait_optimizer()
        out = super()._apply(fn, *a, **k)
        if self._flat is not None and self._flat.adam_m is not None:
            self._adam_carry = (self._flat.adam_m, self._flat.adam_v, self._flat.n)   # optimiser moments survive .to() / .cuda()
        self._flat = None          # parameters were re-created: re-flatten lazily
        self._student_named, self._frozen_key, self._frozen_memo = None, None, {}
        self._engine = None
        return out

    def state_dict(self, *args, **kw):
        if getattr(self, "_engine", None) is not None:
            self._engine.wait_optimizer()     # an update overlapped with the next forward (FusedAdamW.overlap_next_forward) writes these tensors
        return super().state_dict(*args, **kw)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        if getattr(self, "_engine", None) is not None:
            self._engine.wait_optimizer()
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._student_bf16_fresh = False
        self._teacher_bf16_fresh = False
        return out

    def _ensure_engine(self) -> JepaEngine:
        if self._engine is not None and self._flat is not None and self._flat.owns(self):
            return self._engine
        if self._engine is not None:
            self._engine.wait_optimizer()      # a rebuilt engine must not drop an update still in flight on the old one's side stream
        ops.require_gpu()
        if self.device.type != "cuda":
            raise RuntimeError("wavjepa_amd.JEPA computes only on an MI355X: move the module with .cuda() first "
                               "(there is no CPU fallback on the product path)")
        ext = self.extract_audio
        spec = ext.conv_layers_spec
        if hasattr(ext, "cnns"):             # ConvChannelFeatureExtractor: every audio channel through a mono conv stack
            streams, conv_in = ext.in_channels, 1
            prefixes = ["extract_audio.cnns.0."] if ext.weight_sharing else [f"extract_audio.cnns.{c}." for c in range(streams)]
        else:
            streams, conv_in, prefixes = 1, ext.in_channels, ["extract_audio.cnn."]
        self._audio_channels = ext.in_channels
        self._flat = FlatParams(self, self.device, student=is_student)
        carry = getattr(self, "_adam_carry", None)
        if carry is not None:
            if carry[2] != self._flat.n:
                raise RuntimeError("optimiser state exists for a different parameter layout; rebuild the optimiser")
            self._flat.adam_m, self._flat.adam_v = carry[0].to(self.device), carry[1].to(self.device)
            self._adam_carry = None
        cfg = EngineConfig(conv_spec=spec, in_channels=conv_in, streams=streams, conv_prefixes=prefixes, n_samples=self.target_length,
                           d_enc=self.encoder_embedding_dim, h_enc=self.n_encoder_heads, l_enc=self.encoder.num_layers,
                           d_dec=self.decoder_embedding_dim, h_dec=self.n_decoder_heads, l_dec=self.decoder.num_layers,
                           top_k=int(self.hparams.average_top_k_layers), ln_eps=self.encoder.layer_norm_eps,
                           norm_first_enc=self.encoder.norm_first, norm_first_dec=self.decoder.norm_first,
                           conv_mode=getattr(ext, "mode", "default"), conv_bias=bool(getattr(ext, "conv_bias", False)),
                           loss_kind=self.loss_kind, loss_beta=self.loss_beta, recompute=self.use_gradient_checkpointing,
                           dropout_enc=self.encoder.dropout, dropout_dec=self.decoder.dropout,
                           act_enc=self.encoder.activation, act_dec=self.decoder.activation,
                           layerdrop_enc=self.encoder_layerdrop, layerdrop_dec=self.decoder_layerdrop)
        self._engine = JepaEngine(cfg, self._flat, self.pos_encoding_encoder.data, self.pos_encoding_decoder.data)
        self._anchor = torch.zeros(1, device=self.device, requires_grad=True)
        self._student_bf16_fresh = False
        self._teacher_bf16_fresh = False
        return self._engine

    def _prepare_weights(self) -> None:
        eng = self._ensure_engine()
        fresh = self._student_bf16_fresh and self._teacher_bf16_fresh
        self._flat.bf16_fresh = fresh
        eng.prepare_weights()
        # only the fused optimiser / EMA kernels keep the shadows in sync; anything else (a stock torch optimiser,
        # manual edits) changes fp32 masters behind our back, so stay conservative unless they ran.
        self._student_bf16_fresh = False
        self._teacher_bf16_fresh = True

    # ------------------------------------------------------------------------------------------------ schedule / EMA
    def _get_ema_decay(self) -> float:
        if self.global_step >= self.ema_end_step:
            return self.hparams.ema_end_decay
        r = self.hparams.ema_end_decay - self.hparams.ema_decay
        return self.hparams.ema_end_decay - r * (1 - self.global_step / self.ema_end_step)

    @torch.no_grad()
    def _step_teacher(self) -> None:
        self._ensure_engine().ema_step(float(self._get_ema_decay()))
        self._teacher_bf16_fresh = True

    def configure_optimizers(self):
        groups = None
        if self.weight_decay_exclude is not None or self.layer_lr_decay != 1.0:
            from .optim import param_groups
            groups = param_groups(self, weight_decay_exclude=self.weight_decay_exclude, layer_lr_decay=self.layer_lr_decay,
                                  lr=self.hparams.lr, weight_decay=self.hparams.adam_weight_decay)
        optimizer = FusedAdamW(self, lr=self.hparams.lr, betas=self.hparams.adam_betas, eps=self.hparams.adam_eps,
                               weight_decay=self.hparams.adam_weight_decay, groups=groups)
        sched = cosine_schedule_with_warmup(optimizer, num_warmup_steps=int(self.hparams.warmup_steps),
                                            num_training_steps=self._max_steps())
        return {"optimizer": optimizer, "lr_scheduler": {"scheduler": sched, "interval": "step"}}

    # ------------------------------------------------------------------------------------------------ batch preparation
    def on_after_batch_transfer(self, batch, dataloader_idx: int = 0):
        """Random 2.01 s crops, per-crop normalisation, bf16 cast, flatten, shuffle of the audio rows
        (reference jepa.py:275-316).  RNG calls mirror the reference's (torch.randint on the device, torch.randperm on CPU)."""
        audio_batch, ctx_masks, target_indices, ctx_and_target_masks = batch
        if audio_batch.ndim != 3:
            audio_batch = audio_batch.unsqueeze(1)
        self._ensure_engine()
        audio_batch = audio_batch.to(self.device, dtype=torch.float32).contiguous()
        B, C, L_full = audio_batch.shape
        S = self.nr_samples_per_audio
        starts = torch.randint(0, L_full - self.target_length + 1, (B, S), device=self.device)
        idx = torch.randperm(B * S)
        perm_inv = torch.empty_like(idx)
        perm_inv[idx] = torch.arange(B * S)
        out = torch.empty(B * S, C, self.target_length, dtype=torch.bfloat16, device=self.device)
        # (through the page-locked staging ring: a copy from pageable memory would hold the host until the previous step's optimiser
        # kernels have run)
        perm_dev = pack_upload([perm_inv.to(torch.int32).numpy()], self.device)[0]
        ops.crop_normalize_bf16(audio_batch, starts.to(torch.int32), out, B=B, S=S, C=C, L_full=L_full, length=self.target_length,
                                perm_inv=perm_dev)
        return out, self.collate_fn(ctx_masks), self.collate_fn(target_indices), self.collate_fn(ctx_and_target_masks)

    # ------------------------------------------------------------------------------------------------ step
    def training_step(self, batch, batch_idx: int) -> ForwardReturn:
        audio_input, ctx_masks, target_indices, ctx_and_target_masks = batch
        k = accumulate_window(self)
        if k > 1:                      # micro-batch batch_idx % k of its window: dropout counter and monitor (forward)
            self._micro = (int(batch_idx) % k, k)
            try:
                out = self(audio_input, ctx_masks, target_indices, ctx_and_target_masks)
            finally:
                self._micro = (0, 1)
        else:
            out = self(audio_input, ctx_masks, target_indices, ctx_and_target_masks)
        logged = {"train/loss": out["loss"], "ema": self._get_ema_decay()}
        if self.last_kept is not None and self._layerdrop_on():      # LayerDrop: how many layers of each stack ran in this forward
            logged.update({"train/kept_encoder": len(self.last_kept["enc"]), "train/kept_decoder": len(self.last_kept["dec"])})
        self.log_dict(logged, prog_bar=True, sync_dist=True)
        if "pred_var" in out:          # a monitored step (monitor_every)
            self.log_dict({"train/pred_var": out["pred_var"], "train/target_var": out["target_var"]}, prog_bar=False, sync_dist=True)
        self._step_teacher()           # EMA with the pre-update student, before backward (reference jepa.py:330-331)
        return out

    def forward(self, audio: torch.Tensor, ctx_masks, target_indices, ctx_and_target_masks) -> ForwardReturn:
        eng = self._ensure_engine()
        if audio.ndim != 3:
            raise ValueError("audio must be [batch, channels, samples]")
        audio = audio.to(self.device, dtype=torch.bfloat16).contiguous()
        if audio.shape[-1] != self.target_length:
            raise ValueError(f"expected {self.target_length} samples per clip, got {audio.shape[-1]}")
        if audio.shape[1] != self.extract_audio.in_channels:
            raise ValueError(f"expected {self.extract_audio.in_channels} audio channel(s), got {audio.shape[1]}")
        plan = ctx_masks if isinstance(ctx_masks, MaskPlan) else make_mask_plan(ctx_masks, target_indices, ctx_and_target_masks, self.device)
        self._prepare_weights()
        if self.training and torch.is_grad_enabled():      # the frozen set of this step: read again at every training forward
            self._frozen_step = self._frozen_names()
            eng.set_frozen(self._frozen_step)
            eng.grad_mult = self.feature_grad_mult if self.feature_grad_mult > 0 else 1.0
        eng.drop_seed = self._dropout_key()
        every = int(self.monitor_every)
        i, k = self._micro
        # (a window of k micro-batches: the one that closes it is the monitored forward of its optimiser step)
        monitor = self.training and every > 0 and int(self.global_step) % every == 0 and i == k - 1
        drop_call = dropout_call_of(int(self.global_step), k, i, self.dropout_call)
        kept = self._layerdrop_kept(drop_call) if self.training else None
        extra = {} if kept is None else dict(kept=kept)        # (no LayerDrop: the call as it always was)
        if monitor:
            eng.forward(audio, plan, train=self.training, drop_call=drop_call, monitor=True, **extra)
        else:
            eng.forward(audio, plan, train=self.training, drop_call=drop_call, **extra)
        if kept is not None:
            self.last_kept = {s: list(kept.get(s, range(n))) for s, n in (("enc", self.encoder.num_layers), ("dec", self.decoder.num_layers))}
        N, T = audio.shape[0], eng.T
        if torch.is_grad_enabled():
            loss = _EngineLoss.apply(self._anchor, self)
        else:
            loss = eng.loss[0].clone()
        out = _StepOutputs(eng, local_features=eng.lf.view(N, T, -1), contextual_features=eng.cf[:plan.n_ctx], loss=loss,
                           targets=eng.targets.view(N, T, -1))
        if monitor:                    # copies: the engine's buffer is overwritten by the next monitored step
            stats = eng.moments.clone()
            out["pred_var"], out["target_var"] = stats[0], stats[1]
        return out

    # ------------------------------------------------------------------------------------------------ partial training
    def _student(self) -> List[Tuple[str, nn.Parameter]]:
        if self._student_named is None:      # (built once: named_parameters() walks every tensor, FlatParams.owns says what that costs)
            self._student_named = [(n, p) for n, p in self.named_parameters() if is_student(n)]
        return self._student_named

    def freeze(self, *patterns: str) -> List[str]:
        """requires_grad_(False) on the student parameters the fnmatch `patterns` select ("extract_audio.*", "encoder.layers.[0-2].*",
        "*.bias"); returns their names.  A pattern that selects nothing: ValueError.  The teacher is never selected."""
        return self._set_trainable(patterns, False)

    def unfreeze(self, *patterns: str) -> List[str]:
        """requires_grad_(True) on the student parameters the patterns select; returns their names."""
        return self._set_trainable(patterns, True)

    def _set_trainable(self, patterns, flag: bool) -> List[str]:
        named = self._student()
        names = match([n for n, _ in named], patterns)
        hit = set(names)
        for n, p in named:
            if n in hit:
                p.requires_grad_(flag)
                if flag and self._flat is not None and self._flat.owns(self):
                    p.grad = self._flat.g32[self._flat.by_name[n].offset:self._flat.by_name[n].offset + p.numel()].view(p.shape)
                elif not flag:
                    p.grad = None
        if self._flat is not None:           # attach_grads() between now and the next forward must not re-expose a frozen gradient
            self._flat.frozen = (self._flat.frozen - hit) if flag else (self._flat.frozen | hit)
        return names

    def _extractor_held(self) -> bool:
        """extract_audio.* is frozen by an option: feature_grad_mult = 0, or the freeze_feature_extractor_updates schedule"""
        return self.feature_grad_mult == 0.0 or int(self.global_step) < self.freeze_feature_extractor_updates

    def _frozen_names(self) -> frozenset:
        """The frozen student parameters as things stand: requires_grad=False, and extract_audio.* while an option holds it."""
        named = self._student()
        key = (tuple(p.requires_grad for _, p in named), self._extractor_held())
        if key != self._frozen_key:
            if key not in self._frozen_memo:         # (one object per set: the engine and the optimiser key their own tables by it)
                self._frozen_memo[key] = frozenset(n for (n, _), on in zip(named, key[0]) if not on or (key[1] and n.startswith("extract_audio.")))
            self._frozen_key, self._frozen_set = key, self._frozen_memo[key]
        return self._frozen_set

    def _frozen_for_update(self) -> frozenset:
        """What the optimiser holds still: the frozen set of the step whose gradients it applies (before any: as things stand)"""
        return self._frozen_step if self._frozen_step is not None else self._frozen_names()

    @property
    def dropout_seed(self) -> int:
        return self._dropout_seed

    @dropout_seed.setter
    def dropout_seed(self, seed: int) -> None:       # (the checkpoint's hyper-parameters follow: a resumed run reads the seed there)
        self._dropout_seed = int(seed)
        if "dropout_seed" in self.hparams:
            self.hparams["dropout_seed"] = int(seed)

    def _layerdrop_on(self) -> bool:
        return self.encoder_layerdrop > 0 or self.decoder_layerdrop > 0 or bool(self._layerdrop_keep)

    @property
    def layerdrop_keep(self) -> Optional[Dict[str, List[int]]]:
        return self._layerdrop_keep

    @layerdrop_keep.setter
    def layerdrop_keep(self, keep) -> None:
        self._layerdrop_keep = check_keep(keep, dict(enc=self.encoder.num_layers, dec=self.decoder.num_layers))

    def _layerdrop_kept(self, call: int) -> Optional[Dict[str, List[int]]]:
        """stack -> the layers that run in the training forward with dropout call counter `call`: an explicit layerdrop_keep entry, else
        the draw of a stack whose rate is set.  None when neither is set (the generator is not evaluated and the engine is called as
        it always was).  The generator's key is dropout_seed itself, without the rank: all ranks skip the same layers."""
        fixed = self._layerdrop_keep or {}
        rates = dict(enc=(self.encoder_layerdrop, self.encoder.num_layers), dec=(self.decoder_layerdrop, self.decoder.num_layers))
        out = {}
        for s, (p, n) in rates.items():
            if s in fixed:
                out[s] = list(fixed[s])
            elif p > 0:
                out[s] = kept_layers(self.dropout_seed, call, s, n, p)
        return out or None

    def _dropout_key(self) -> int:
        """The generator's 64-bit key: dropout_seed with the data-parallel rank mixed in (every rank draws its own masks)."""
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        return (int(self.dropout_seed) ^ (rank * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF

    @torch.no_grad()
    def get_audio_representation(self, audio: torch.Tensor, padding_mask: Optional[torch.Tensor]) -> torch.Tensor:
        """Student-only inference (reference jepa.py:456-467): [B, C, L] -> [B, T, d_enc] fp32."""
        self.eval()
        eng = self._ensure_engine()
        audio = audio.to(self.device, dtype=torch.bfloat16).contiguous()
        self._prepare_weights()
        mask = None if padding_mask is None else padding_mask.to(self.device).to(torch.uint8).contiguous()
        return eng.infer(audio, mask).clone()
