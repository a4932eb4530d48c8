"""Reference of gradient accumulation (accumulate_grad_batches = k), composed from the oracle's own pieces (oracle/jepa_oracle.py) in
the order pytorch_lightning's automatic optimisation gives the reference: per micro-batch a forward, the teacher's EMA with the decay
of the current global step (reference jepa.py:330-331 runs inside training_step) and (loss / k).backward() into the SAME .grad tensors;
behind the k-th one global-norm clip of the sum, one AdamW update at the learning rate of the optimiser step.  At k = 1 it performs
J.train_step's operations one for one.  Also the host arithmetic of the dropout call counter, stated independently of the package."""
from typing import Dict, List, Optional

from oracle import jepa_oracle as J


def train_window(P, opt_state, step: int, batches, k: Optional[int] = None, *, lr: float = 4e-4, warmup: int = 100000,
                 total_steps: int = 375000, betas=(0.9, 0.98), eps: float = 1e-6, weight_decay: float = 0.04, clip: float = 5.0,
                 ema=(0.999, 0.99999, 100000), mode: str = "fp32", **fw) -> Dict[str, object]:
    """One optimiser step `step` over the micro-batches `batches` (each (audio, ctx, tgt, vis)), every loss scaled by 1 / k.  k defaults
    to len(batches); fewer batches than k is the window the loader ended in (Lightning's last-batch rule: the parts keep 1 / k)."""
    k = len(batches) if k is None else k
    assert 1 <= len(batches) <= k
    names = J.trainable_names(P)
    for n in names:
        P[n].requires_grad_(True)
        P[n].grad = None
    losses: List[float] = []
    r = J.ema_decay(step, *ema)
    for audio, ctx, tgt, vis in batches:
        out = J.jepa_forward(P, audio, ctx, tgt, vis, mode=mode, **fw)
        J.ema_update(P, r)                       # per micro-batch, with the pre-update student
        (out["loss"] / k).backward()             # autograd adds into P[n].grad
        losses.append(float(out["loss"].detach()))
    grads = {n: P[n].grad.detach().clone() for n in names if P[n].grad is not None}
    for n in names:
        P[n].requires_grad_(False)
        P[n].grad = None
    gnorm = J.clip_grad_norm(grads, clip)
    J.adamw_update(P, grads, opt_state, step + 1, lr * J.lr_lambda(step, warmup, total_steps), betas, eps, weight_decay)
    return dict(losses=losses, loss=sum(losses) / len(losses), grad_norm=gnorm, ema=r)


def micro_index(batch_idx: int, k: int) -> int:
    return batch_idx % k


def dropout_call(global_step: int, k: int, micro: int, explicit: Optional[int] = None) -> int:
    """The dropout generator's 32-bit call counter of micro-batch `micro` of optimiser step `global_step`: an explicit value wins, else
    global_step * k + micro (k = 1: global_step); a counter that does not fit 32 bits is refused."""
    if explicit is not None:
        return explicit
    call = global_step * k + micro
    if k > 1 and call > 0xFFFFFFFF:
        raise OverflowError(call)
    return call
