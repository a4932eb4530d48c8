"""LayerDrop for the oracle.  TEST INFRASTRUCTURE ONLY (a helper, not a test).

`oracle/jepa_oracle.py` walks every layer of a stack; its callers look `encoder_stack` up as a module global on every call.
`install(monkeypatch, kept)` puts a walker in its place that runs only the listed layers of the listed stacks -- fairseq's
TransformerEncoder under LayerDrop: a skipped layer passes the stream unchanged, nothing is rescaled, the final norm always runs, an
empty list leaves the final norm over the stack's input.  `kept` maps the ENGINE's stack names to sorted layer indices
({"enc": [...], "dec": [...]}: "encoder" / "decoder" in the oracle's parameter names); a stack that is not named, and always the
teacher ("teacher_encoder"), runs every layer.  The walker calls `J.post_norm_layer` through the module as the oracle does, with the
layer's OWN parameter prefix, so it composes with tests/prenorm_reference.py (a pre-norm layer in that place) and with
tests/dropout_reference.py (whose mask provider reads the layer index out of the prefix: the masks of layer kept[j] are asked for by
kept[j], not by the walk position j).

`kept` is read at every call, so a test may change the dict between forwards (drawn sets: one per step).

`train_window` is tests/accumulate_reference.py's window with one kept set per micro-batch and the engine's gradient semantics: a
parameter no backward reached has gradient ZERO, not None -- it enters the clip norm as 0 and AdamW still applies weight decay and
decays its moments (what a layer receives under DDP; INTEGRATION.md, differences by design).  `kept_sets` restates how the product
draws (wavjepa_amd/layerdrop.py's generator through tests/dropout_reference.py's own Philox).
"""
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from oracle import jepa_oracle as J
from tests import dropout_reference as R

STACK_OF = dict(encoder="enc", decoder="dec")       # oracle stack name -> engine stack name
SITE_LAYER = 5
_ENCODER_STACK = J.encoder_stack                    # the oracle's own walker, whatever a test patches into the module later


def layerdrop_stack(kept: Dict[str, Sequence[int]]):
    """A walker for J.encoder_stack's place (see the module docstring)."""
    def encoder_stack(P, stack, x, nhead, key_mask, mode, final_norm=True, eps=1e-6, keep=None, keep_last=0):
        L = J.n_layers(P, stack)
        run = kept.get(STACK_OF.get(stack))
        for i in (range(L) if run is None else run):
            x = J.post_norm_layer(P, f"{stack}.layers.{i}.", x, nhead, key_mask, mode, eps)
            if keep is not None and L - i <= keep_last:
                keep.append(x)
        if final_norm:
            x = J._ln(x, P[f"{stack}.norm.weight"], P[f"{stack}.norm.bias"], 1e-5)
        return x
    return encoder_stack


def install(monkeypatch, kept: Dict[str, Sequence[int]]) -> None:
    monkeypatch.setattr(J, "encoder_stack", layerdrop_stack(kept))


def skipped_names(P, kept: Dict[str, Sequence[int]]) -> List[str]:
    """The parameters of the layers that do not run under `kept`."""
    out = []
    for stack, s in STACK_OF.items():
        if kept.get(s) is None:
            continue
        gone = set(range(J.n_layers(P, stack))) - set(kept[s])
        out += [n for n in P if any(n.startswith(f"{stack}.layers.{i}.") for i in gone)]
    return out


def draw(seed: int, call: int, stack: int, layer: int) -> int:
    """The 16-bit keep draw of one layer: Philox counter (0, 0, 5 | layer << 8 | stack << 16, call), key = the seed, draw 0."""
    w0 = R.philox4x32_10(0, 0, R.stream_id(stack, layer, SITE_LAYER), call & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return int(w0) & 0xFFFF


def kept_set(seed: int, call: int, stack: str, n_layers: int, p: float) -> List[int]:
    thr = int(np.floor(p * 65536.0 + 0.5))
    return [i for i in range(n_layers) if draw(seed, call, R.STACK[stack], i) >= thr]


def kept_sets(seed: int, call: int, layers: Dict[str, int], rates: Dict[str, float]) -> Dict[str, List[int]]:
    return {s: kept_set(seed, call, s, layers[s], rates[s]) for s in layers if rates.get(s)}


def train_window(P, opt_state, step: int, batches, kept_per_batch, kept: Dict[str, Sequence[int]], k: Optional[int] = None, *,
                 lr: float = 4e-4, warmup: int = 100000, total_steps: int = 375000, betas=(0.9, 0.98), eps: float = 1e-6,
                 weight_decay: float = 0.04, clip: float = 5.0, ema=(0.999, 0.99999, 100000), mode: str = "fp32", **fw):
    """One optimiser step over the micro-batches `batches`, micro-batch j under kept_per_batch[j] (written into `kept`, the dict the
    installed walker reads).  k = 1 with every layer listed performs J.train_step's operations one for one."""
    k = len(batches) if k is None else k
    assert 1 <= len(batches) <= k and len(kept_per_batch) == len(batches)
    names = J.trainable_names(P)
    for n in names:
        P[n].requires_grad_(True)
        P[n].grad = None
    losses: List[float] = []
    r = J.ema_decay(step, *ema)
    for (audio, ctx, tgt, vis), sets in zip(batches, kept_per_batch):
        kept.clear()
        kept.update(sets)
        out = J.jepa_forward(P, audio, ctx, tgt, vis, mode=mode, **fw)
        J.ema_update(P, r)
        (out["loss"] / k).backward()
        losses.append(float(out["loss"].detach()))
    grads = {n: (torch.zeros_like(P[n]) if P[n].grad is None else P[n].grad.detach().clone()) for n in names}
    for n in names:
        P[n].requires_grad_(False)
        P[n].grad = None
    gnorm = J.clip_grad_norm(grads, clip)
    J.adamw_update(P, grads, opt_state, step + 1, lr * J.lr_lambda(step, warmup, total_steps), betas, eps, weight_decay)
    return dict(losses=losses, loss=sum(losses) / len(losses), grad_norm=gnorm, ema=r)
