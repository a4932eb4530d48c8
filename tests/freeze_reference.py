"""Reference of partial training, composed from the oracle's own pieces (oracle/jepa_oracle.py): a step in which the frozen names
carry requires_grad=False -- autograd then neither differentiates them nor walks below the lowest trainable tensor -- fairseq's
GradMultiply as a custom autograd function on the conv output (in front of feature_norms), and an optimiser loop that skips the
parameters without gradient, as torch.optim.AdamW does.  Written the way tests/accumulate_reference.py handles P[n].requires_grad_."""
import contextlib
import fnmatch
from typing import Dict, Iterable, List, Sequence

import torch

from oracle import jepa_oracle as J

SETS = {
    "A": ["extract_audio.*"],
    "B": ["extract_audio.*", "feature_norms.*", "post_extraction_mapper.*", "encoder.layers.[0-2].*"],
    "C": ["*.bias", "decoder.layers.1.*"],
    "D": ["mask_token", "extract_audio.*", "feature_norms.*", "post_extraction_mapper.*", "encoder.*"],   # all but decoder.* and the two mappers
}


def frozen_names(names: Iterable[str], patterns: Sequence[str]) -> List[str]:
    return [n for n in names if any(fnmatch.fnmatchcase(n, p) for p in patterns)]


class GradMultiply(torch.autograd.Function):
    """fairseq.modules.GradMultiply: identity forward, gradient times `scale` (in the gradient's own dtype: bf16 under the bf16 flow)"""

    @staticmethod
    def forward(ctx, x, scale):
        ctx.scale = scale
        return x.view_as(x)

    @staticmethod
    def backward(ctx, grad):
        return grad * ctx.scale, None


@contextlib.contextmanager
def feature_grad_mult(m: float):
    """Inside: the oracle's conv front-end hands its output through GradMultiply(m) (m = 1: untouched)."""
    real = J.conv_frontend
    if m != 1.0:
        J.conv_frontend = lambda *a, **k: GradMultiply.apply(real(*a, **k), m)
    try:
        yield
    finally:
        J.conv_frontend = real


def grads(P: Dict[str, torch.Tensor], audio, ctx, tgt, vis, frozen: Iterable[str] = (), m: float = 1.0, mode: str = "bf16", **fw):
    """(forward dict, {name: gradient} of the trainable names) on detached copies of P; a frozen name has no entry"""
    frozen = set(frozen)
    Q = {k: v.detach().clone() for k, v in P.items()}
    names = [n for n in J.trainable_names(Q) if n not in frozen]
    for n in names:
        Q[n].requires_grad_(True)
    with feature_grad_mult(m):
        out = J.jepa_forward(Q, audio.float() if mode == "fp32" else audio, ctx, tgt, vis, mode=mode, **fw)
        if names:
            out["loss"].backward()
    for n in J.trainable_names(Q):
        assert (Q[n].grad is None) == (n in frozen or not names), n
    return out, {n: Q[n].grad for n in names}


def train_step(P, opt_state, step: int, batch, frozen: Iterable[str] = (), m: float = 1.0, *, lr: float = 4e-4, warmup: int = 100000,
               total_steps: int = 375000, betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.04, clip: float = 5.0,
               ema=(0.999, 0.99999, 100000), mode: str = "fp32", **fw) -> Dict[str, float]:
    """J.train_step with the frozen names left out of autograd: no gradient, no moments, no update, no weight decay for them; the
    clipped norm is the norm over the trainable gradients."""
    audio, ctx, tgt, vis = batch
    frozen = set(frozen)
    names = [n for n in J.trainable_names(P) if n not in frozen]
    for n in names:
        P[n].requires_grad_(True)
        P[n].grad = None
    with feature_grad_mult(m):
        out = J.jepa_forward(P, audio, ctx, tgt, vis, mode=mode, **fw)
        r = J.ema_decay(step, *ema)
        J.ema_update(P, r)
        if names:
            out["loss"].backward()
    got = {n: P[n].grad.detach().clone() for n in names if P[n].grad is not None}
    for n in names:
        P[n].requires_grad_(False)
        P[n].grad = None
    gnorm = J.clip_grad_norm(got, clip)
    J.adamw_update(P, got, opt_state, step + 1, lr * J.lr_lambda(step, warmup, total_steps), betas, eps, weight_decay)
    return dict(loss=float(out["loss"].detach()), grad_norm=gnorm, ema=r)
