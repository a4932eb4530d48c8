"""fp64 reference, per-element bounds, fp32 emulation, mutations and the oracle-side objective of the masked-loss family
(wj_masked_loss: mse, l1, smooth_l1(beta), huber(delta)).  Test infrastructure; used by tests/test_masked_loss_cpu.py and
tests/test_masked_loss_gpu.py.  Style and constants are those of tests/norm_reference.py (U = 2^-24, KAPPA, bf16_bound); kind "mse"
IS norm_reference.masked_mse.

What the kernel documents (include/wavjepa_hip.h: wj_loss_args), with d = fl32(p - y), ad = |d|, sg = sign(d) (sign(0) = 0):
    l1         e = ad                                             e' = sg
    smooth_l1  ib = fl32(1 / beta), q = fl32(d ib)
               e = ad < beta ? fl32(fl32(0.5 d) q) : fl32(ad - 0.5 beta)        e' = ad < beta ? q : sg
    huber      e = ad <= beta ? fl32(fl32(0.5 d) d) : fl32(beta fl32(ad - 0.5 beta))   e' = ad <= beta ? d : beta sg
    row        err = (lane sums of e in column order, wave butterfly) / D;  loss[0] = (sum of rows, one workgroup) / (count + 1e-8)
    dpreds     bf16(fl32(e' gk)),  gk = 1 / (D (count + 1e-8)) * gscale * gscale_ptr[0]   (four fp32 operations)

Bounds, first order, relative to the exact e (or e') of the exact difference p - y.  The subtraction leaves d with relative error u;
|d e'(d)| <= 2 e holds for every kind and branch (l1: = e; quadratic branches: = 2 e; linear branches: ad <= 2 (ad - 0.5 beta) because
ad >= beta), so d costs 2 u e (u e for l1).  0.5 d, 0.5 beta and beta sg are exact (powers of two / a sign).  Then, per operation one u:
    l1         d 1                                              + /D 1                      = 2
    smooth_l1  quadratic: d 2 + ib 1 + d ib 1 + product 1 = 5;  linear: d 2 + subtraction 1 = 3 (the subtraction's result is >= ad / 2:
               no cancellation);  the larger, + select 1        + /D 1                      = 7
    huber      quadratic: d 2 + product 1 = 3;  linear: d 2 + subtraction 1 + product 1 = 4;  + select 1 + /D 1 = 6
The select's u: a d within u of the knot may take the other branch than the exact difference does; the branches agree there in value
and slope, so the disagreement is second order -- one u covers it with room.  A row: derr = (KAPPA + E_OPS) u err, KAPPA u for the sum
over the row (any order, fused or not); the loss: KAPPA u sum|err| + sum derr over den, + 2 u |loss| for the division and the
denominator (norm_reference.masked_mse's form).
dpreds in front of the bf16 rounding: gk and the product e' gk take 6 u (norm_reference's constant, which there includes d); e' adds
    l1 0 (the sign is exact)      smooth_l1 d 1 + ib 1 + product 1 + select 1 = 4      huber d 1 + select 1 = 2
and bf16_bound does the rounding.  Where d = 0 exactly every kind has e' = 0 and the bound is 0: sign(0) = 1 is rejected outright.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F_

from tests import norm_reference as nr
from tests.norm_reference import KAPPA, U, Pair, bf16, bf16_bound, f64

F = np.float32
KINDS = ("mse", "l1", "smooth_l1", "huber")
BETAS = (0.25, 1.0, 2.0)
E_OPS = {"l1": 2, "smooth_l1": 7, "huber": 6}
G_OPS = {"l1": 6, "smooth_l1": 10, "huber": 8}
GRID = [("mse", 1.0), ("l1", 1.0)] + [(k, b) for k in ("smooth_l1", "huber") for b in BETAS]       # every kind x beta of the tests


def f32beta(beta: float) -> float:
    """beta as the kernel sees it (a float field of the argument struct)"""
    return float(np.float32(beta))


def elem(kind: str, d: torch.Tensor, beta: float = 1.0, how: str = ""):
    """(e(d), e'(d)) in the dtype of d.  `how` names a WRONG formula (the mutations): "sign0", "factor2", "no_inv_beta", "no_half",
    "no_delta"."""
    ad, sg = d.abs(), torch.sign(d)
    if kind == "mse":
        return d * d, 2 * d
    if kind == "l1":
        if how == "sign0":
            return ad, torch.where(d == 0, torch.ones_like(d), sg)
        return ad, (2 * sg if how == "factor2" else sg)
    if kind == "smooth_l1":
        ib = 1.0 if how == "no_inv_beta" else 1.0 / beta
        half = 1.0 if how == "no_half" else 0.5
        quad = ad < beta
        return torch.where(quad, half * d * d * ib, ad - half * beta), torch.where(quad, (2 * half) * d * ib, sg)
    if kind == "huber":
        k = 1.0 if how == "no_delta" else beta
        quad = ad <= beta
        return torch.where(quad, 0.5 * d * d, k * (ad - 0.5 * beta)), torch.where(quad, d, k * sg)
    raise ValueError(kind)


def _rows(preds, targets, tgt, B, G, T, D, rows):
    p = f64(preds).reshape(-1, D)
    y = f64(targets).reshape(B, T, D)
    on_dense = (tgt.detach().cpu().reshape(-1) != 0)
    dense = torch.arange(B * G * T) if rows is None else rows.detach().cpu().long()
    p = p[:dense.numel()]
    count = float(on_dense.sum())
    on = on_dense[dense].double()[:, None]
    b, t = (dense // T) // G, dense % T
    return (p - y[b, t]), on, count


def masked_loss(preds, targets, tgt, B: int, G: int, T: int, D: int, kind: str, beta: float = 1.0, gscale: float = 1.0,
                gscale_dev: Optional[float] = None, rows: Optional[torch.Tensor] = None, how: str = "") -> Dict[str, Pair]:
    """wj_masked_loss: {"loss": (ref [2], bound), "dpreds": (ref bf16 values [R][D], bound), "_on": target rows}.  loss[1] = count is
    exact; dpreds is exactly zero on rows that are not targets; "_v" (not for mse) is dpreds in front of the bf16 rounding.
    `how`: a wrong formula (see elem) -- the reference of a mutation."""
    if kind == "mse" and not how:
        return nr.masked_mse(preds, targets, tgt, B, G, T, D, gscale, gscale_dev, rows)
    beta = f32beta(beta)
    d, on, count = _rows(preds, targets, tgt, B, G, T, D, rows)
    den = count + float(np.float32(1e-8))
    e, g = elem(kind, d, beta, how)
    err = (e * on).mean(1)
    derr = (KAPPA + E_OPS[kind]) * U * err
    loss0 = err.sum() / den
    b0 = (KAPPA * U * err.abs().sum() + derr.sum()) / den + 2 * U * abs(loss0)
    gk = 1.0 / (D * den) * float(np.float32(gscale)) * (1.0 if gscale_dev is None else float(np.float32(gscale_dev)))
    v = g * on * gk
    return {"loss": (torch.stack([loss0, torch.tensor(count, dtype=torch.float64)]), torch.stack([b0, torch.tensor(0.0, dtype=torch.float64)])),
            "dpreds": (bf16(v), bf16_bound(v, G_OPS[kind] * U * v.abs()) * on), "_on": (on[:, 0], on[:, 0]), "_v": (v, torch.zeros_like(v))}


# ------------------------------------------------------------------------------------------------------------ emulation
def emulate_masked_loss(preds, targets, tgt, B, G, T, D, kind, beta=1.0, gscale=1.0, gscale_dev=None, rows=None) -> Dict[str, np.ndarray]:
    """fp32 numpy in the kernel's documented order (modelled on norm_reference.emulate_masked_mse, which kind "mse" is)"""
    if kind == "mse":
        return nr.emulate_masked_mse(preds, targets, tgt, B, G, T, D, gscale, gscale_dev, rows)
    beta = F(beta)
    p = preds.float().numpy().reshape(-1, D)
    y = targets.numpy().astype(F).reshape(B, T, D)
    on_dense = (tgt.reshape(-1) != 0).numpy()
    dense = np.arange(B * G * T) if rows is None else rows.numpy().astype(np.int64)
    R = len(dense)
    p = p[:R]
    count = F(on_dense.sum())
    den = (count + F(1e-8)).astype(F)
    gk = F(1.0) / (F(D) * den).astype(F)
    gk = (gk * F(gscale)).astype(F)
    gk = (gk * (F(1.0) if gscale_dev is None else F(gscale_dev))).astype(F)
    on = on_dense[dense]
    b, t = (dense // T) // G, dense % T
    d = ((p - y[b, t]).astype(F) * on[:, None]).astype(F)
    ad, sg = np.abs(d), np.sign(d).astype(F)
    if kind == "l1":
        le, lg = ad, sg
    elif kind == "smooth_l1":
        ib = (F(1.0) / beta).astype(F)
        q = (d * ib).astype(F)
        quad = ad < beta
        le = np.where(quad, ((F(0.5) * d).astype(F) * q).astype(F), (ad - F(0.5) * beta).astype(F))
        lg = np.where(quad, q, sg)
    elif kind == "huber":
        quad = ad <= beta
        le = np.where(quad, ((F(0.5) * d).astype(F) * d).astype(F), (beta * (ad - F(0.5) * beta).astype(F)).astype(F))
        lg = np.where(quad, d, (beta * sg).astype(F))
    else:
        raise ValueError(kind)
    le = (le * on[:, None]).astype(F)
    lanes = np.zeros((R, 64), dtype=F)
    for c0 in range(0, D, 256):
        blk = np.zeros((R, 256), dtype=F)
        w = min(256, D - c0)
        blk[:, :w] = le[:, c0:c0 + w]
        blk = blk.reshape(R, 64, 4)
        for e in range(4):
            lanes = (lanes + blk[:, :, e]).astype(F)
    err = (nr._butterfly(lanes) / F(D)).astype(F) if R else np.zeros(0, dtype=F)
    acc = np.zeros(1024, dtype=F)                    # mse_final_kernel: thread t adds rows t, t + 1024, ...; then block_sum
    for i in range(0, R, 1024):
        seg = np.zeros(1024, dtype=F)
        seg[:len(err[i:i + 1024])] = err[i:i + 1024]
        acc = (acc + seg).astype(F)
    waves = nr._butterfly(acc.reshape(16, 64))
    tot = F(0)
    for w in range(16):
        tot = F(tot + waves[w])
    dp = torch.from_numpy(((lg * on[:, None]).astype(F) * gk).astype(F)).to(torch.bfloat16).float().numpy()
    return {"loss": np.array([F(tot / den), count], dtype=F), "dpreds": dp}


# ------------------------------------------------------------------------------------------------------------ cases
def plant(c: dict, B: int, G: int, T: int, D: int, beta: float) -> dict:
    """A copy of nr.mse_inputs' case with two elements of the first target row (row 0 when there is none) set so that p == y exactly
    (column 0) and |p - y| == beta exactly in fp32 (column 1).  Targets are shared by the G groups of a clip: only that row's clip and
    token are edited."""
    c = {k: v.clone() for k, v in c.items()}
    on = torch.nonzero(c["tgt"].reshape(-1) != 0)
    r = int(on[0]) if on.numel() else 0
    b, t = (r // T) // G, r % T
    p = c["preds"].reshape(-1, D)[r].float()
    y = c["targets"].reshape(B, T, D)
    y[b, t, 0] = p[0]
    y[b, t, 1] = p[1] - np.float32(beta)
    d = p[:2] - y[b, t, :2]
    assert float(d[0]) == 0.0 and abs(float(d[1])) == float(np.float32(beta)), d
    c["planted"] = (r, b, t)
    return c


def quadratic_share(c: dict, B: int, G: int, T: int, D: int, beta: float):
    """(target elements, share of them with |d| < beta)"""
    d, on, _ = _rows(c["preds"], c["targets"], c["tgt"], B, G, T, D, None)
    sel = d[on[:, 0] != 0]
    n = sel.numel()
    return n, (float((sel.float().abs() < np.float32(beta)).double().mean()) if n else 0.0)


# ------------------------------------------------------------------------------------------------------------ mutations
def mutations(got: Dict[str, torch.Tensor], c: dict, B, G, T, D, kind, beta, **kw):
    """[(label, output, mutated copy)] of a correct output `got` ({"loss", "dpreds"}): each wrong formula that applies to the kind moves
    the output by (wrong reference - right reference); dpreds on a non-target row.  Every one must be rejected by masked_loss's bounds."""
    right = masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, **kw)
    hows = {"l1": ("sign0", "factor2"), "smooth_l1": ("no_inv_beta", "no_half"), "huber": ("no_delta",), "mse": ()}[kind]
    out = []
    for how in hows:
        wrong = masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, how=how, **kw)
        for k in ("loss", "dpreds"):
            if not torch.equal(wrong[k][0], right[k][0]):
                out.append((how, k, nr._delta(got[k], right[k][0], wrong[k][0])))
    m = nr.mutate_dpreds_offrow(got["dpreds"], right["_on"][0])
    if m is not None:
        out.append(("dpreds on a non-target row", "dpreds", m))
    return out


# ------------------------------------------------------------------------------------------------------------ oracle side
def oracle_masked_loss(kind: str, beta: float = 1.0) -> Callable:
    """Stands in for oracle.jepa_oracle.masked_mse: the reference's masked_loss (jepa.py:335-362) with
    torch.nn.{MSE, L1, SmoothL1, Huber}Loss(reduction='none') as its loss_fn, in fp32 as autocast runs these losses."""
    fn = {"mse": F_.mse_loss, "l1": F_.l1_loss, "smooth_l1": lambda a, b, reduction: F_.smooth_l1_loss(a, b, reduction=reduction, beta=beta),
          "huber": lambda a, b, reduction: F_.huber_loss(a, b, reduction=reduction, delta=beta)}[kind]

    def masked(preds: torch.Tensor, targets: torch.Tensor, target_indices: torch.Tensor) -> torch.Tensor:
        B, G, T = target_indices.shape
        D = preds.shape[-1]
        p = preds.float().view(B, G, T, D)
        per_pos = fn(p, targets.float()[:, None].expand_as(p), reduction="none").mean(dim=-1) * target_indices
        return per_pos.sum() / (target_indices.sum() + 1e-8)
    return masked


def torch_loss_module(kind: str, beta: float = 1.0):
    nn = torch.nn
    return {"mse": lambda: nn.MSELoss(reduction="none"), "l1": lambda: nn.L1Loss(reduction="none"),
            "smooth_l1": lambda: nn.SmoothL1Loss(reduction="none", beta=beta), "huber": lambda: nn.HuberLoss(reduction="none", delta=beta)}[kind]()
