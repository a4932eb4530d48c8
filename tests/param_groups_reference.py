"""Reference, bounds, layouts, mutations and an fp32 emulation for the AdamW pass with parameter groups (wj_adamw_groups_step,
include/wavjepa_hip_optim.h; test infrastructure of tests/test_param_groups_cpu.py, test_param_groups_ops_gpu.py, test_param_groups_gpu.py).

The reference is tests/optimizer_reference.adamw_step -- the fp64 step and the per-element bound wj_adamw_step is held to, unchanged --
applied group by group: the elements of group k with group k's lr and weight decay, everything else (betas, eps, bias corrections, the
clip coefficient from the ONE global sum of squares) common.  The element-to-group map is brute force: every slot of the flat layout
writes its group over its elements and its padding, one element at a time; the granule map is read off it.

Mutations (a wrong lookup, evaluated in fp64 and applied as a delta to an accepted output, optimizer_reference's way):
  map shifted        the granule map moved by one granule
  offset ignored     a launch on [lo, hi) reads the map from granule 0 instead of lo / 8
  lr swapped         two groups' learning rates exchanged          wd swapped     two groups' weight decays exchanged
  group 0 everywhere every element updated with group 0's pair
  decay from base lr p *= 1 - lr_base * wd[k] instead of 1 - lr[k] * wd[k]
A mutation is CLAIMED where the reference alone separates it: it moves some element by more than 2x its bound.  GROUP_VALUES are
chosen so that each is: weight decay 0 against 0.4 moves p by lr * 0.4 * |p| ~ 4e-4 |p| (bound ~ 1e-7 |p|), learning rates 1e-3
against 1e-5 change the update by two decades.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests import optimizer_reference as orf
from tests.norm_reference import f32eps, f64

GRANULE = 8
MAX_GROUPS = 64
BASE_LR = 4e-4            # the constructor-level lr of the "decay from base lr" mutation: no group's own
# (lr, weight decay) of the first groups of a test layout; further groups repeat them scaled (group_values)
GROUP_VALUES = ((1e-3, 0.4), (1e-5, 0.0), (3e-4, 0.04))
COMMON = dict(beta1=0.9, beta2=0.98, eps=1e-6, max_norm=5.0)
MUTATIONS = ("map shifted", "offset ignored", "lr swapped", "wd swapped", "group 0 everywhere", "decay from base lr")

Pair = Tuple[torch.Tensor, torch.Tensor]


def group_values(n_groups: int) -> Tuple[List[float], List[float]]:
    """lr[k], wd[k]: the three pairs above, each further round of three with the lr scaled by 0.9 (all pairs distinct)"""
    lr = [GROUP_VALUES[k % 3][0] * 0.9 ** (k // 3) for k in range(n_groups)]
    wd = [GROUP_VALUES[k % 3][1] for k in range(n_groups)]
    return lr, wd


def hyper(lr: float, wd: float) -> dict:
    """an optimizer_reference.HYPER entry for one group"""
    return dict(COMMON, lr=lr, weight_decay=wd)


def common_fields(step: int, grad_scale: float = 1.0, max_norm: Optional[float] = None) -> dict:
    """the float fields of wj_adamw_groups_args that all groups share (optimizer_reference.fields without lr / weight_decay)"""
    Fd = orf.fields(hyper(0.0, 0.0), step, grad_scale, max_norm)
    del Fd["lr"], Fd["weight_decay"]
    return Fd


# ------------------------------------------------------------------------------------------------------------ the map, brute force
def element_groups(slots, assignment: Dict[str, int], n: int) -> torch.Tensor:
    """int64 [n]: the group of every element of the flat buffer; a slot's padding up to the next granule is its own.  -1: no slot."""
    out = [-1] * n
    for s in slots:
        k = int(assignment[s.name])
        end = s.offset + s.numel
        while end % GRANULE:
            end += 1
        for i in range(s.offset, end):
            assert out[i] == -1, f"slots overlap at element {i}"
            out[i] = k
    return torch.tensor(out, dtype=torch.int64)


def granule_map(elem: torch.Tensor) -> torch.Tensor:
    """uint8 [n / 8] from the element map: every granule must hold one group"""
    g = elem.view(-1, GRANULE)
    assert bool((g == g[:, :1]).all()) and bool((g >= 0).all()) and bool((g < 256).all()), "a granule holds two groups, or none"
    return g[:, 0].to(torch.uint8)


def layout(kind: str, granules: int) -> Tuple[torch.Tensor, int]:
    """(uint8 [granules], n_groups) of a test layout: one | alt2 (alternating every granule) | runs3 (runs of 1, 48, 129 granules of
    groups 0, 1, 2, repeated) | all64 (granule i in group i % 64) | absent (groups 0 and 2 alternate in runs of 3; group 1 of 3 owns
    nothing)"""
    i = torch.arange(granules)
    if kind == "one":
        return torch.zeros(granules, dtype=torch.uint8), 1
    if kind == "alt2":
        return (i % 2).to(torch.uint8), 2
    if kind == "runs3":
        j = i % 178
        return ((j >= 1).long() + (j >= 49).long()).to(torch.uint8), 3
    if kind == "all64":
        return (i % 64).to(torch.uint8), 64
    if kind == "absent":
        return (2 * ((i // 3) % 2)).to(torch.uint8), 3
    raise ValueError(kind)


LAYOUTS = ("one", "alt2", "runs3", "all64", "absent")


# ------------------------------------------------------------------------------------------------------------ reference
def grouped_step(p, g, m, v, sumsq, Fc: dict, lr: Sequence[float], wd: Sequence[float], elem: torch.Tensor, zero_grad: bool = False) -> Dict[str, Pair]:
    """optimizer_reference.adamw_step per group: p, g, m, v f32 [n], elem int64 [n] the group of each element; Fc common_fields(...)"""
    p, g, m, v = (t.detach().cpu() for t in (p, g, m, v))
    n = p.numel()
    out = {k: (torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)) for k in ("p", "m", "v", "p_bf16", "g")}
    seen = torch.zeros(n, dtype=torch.bool)
    for k in sorted(set(elem.tolist())):
        assert 0 <= k < len(lr), f"element group {k} outside the {len(lr)} groups"
        idx = (elem == k).nonzero().flatten()
        Fd = dict(Fc, lr=f32eps(lr[k]), weight_decay=f32eps(wd[k]))
        r = orf.adamw_step(p[idx], g[idx], m[idx], v[idx], sumsq, Fd, zero_grad=zero_grad)
        for name, (ref, bound) in r.items():
            out[name][0][idx] = ref
            out[name][1][idx] = bound
        seen[idx] = True
    assert bool(seen.all())
    return out


def _p_with(p, g, m, v, sumsq, Fc, lr_e: torch.Tensor, wd_e: torch.Tensor, decay_lr_e: Optional[torch.Tensor] = None) -> torch.Tensor:
    """p' in fp64 with a learning rate and a weight decay PER ELEMENT (the float values the kernel would see); decay_lr_e: the lr
    inside 1 - lr wd, where it differs"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    r = orf._adamw(p, g, m, v, sumsq, dict(Fc, lr=lr_e, weight_decay=wd_e))
    if decay_lr_e is None:
        return r["p"]
    return p * (1.0 - decay_lr_e * wd_e) - r["upd"]


def _f32(vals: Sequence[float]) -> torch.Tensor:
    return torch.tensor([f32eps(x) for x in vals], dtype=torch.float64)


def mutations(p, g, m, v, sumsq, Fc, lr, wd, emap: torch.Tensor, lo: int, n: int, got_p: torch.Tensor, bound_p: torch.Tensor,
              pair: Tuple[int, int] = (0, 1)) -> List[tuple]:
    """[(label, mutated p, claimed)] for a launch on [lo, lo + n) of a buffer whose whole element map is emap; p, g, m, v, got_p,
    bound_p are the launch's own n elements.  pair: the two groups whose values are exchanged."""
    lr32, wd32 = _f32(lr), _f32(wd)
    elem = emap[lo:lo + n]
    right = _p_with(p, g, m, v, sumsq, Fc, lr32[elem], wd32[elem])
    a, b = pair
    swap = torch.arange(len(lr))
    swap[a], swap[b] = b, a
    shifted = torch.roll(emap, GRANULE)[lo:lo + n]
    wrong = {
        "map shifted": _p_with(p, g, m, v, sumsq, Fc, lr32[shifted], wd32[shifted]),
        "offset ignored": _p_with(p, g, m, v, sumsq, Fc, lr32[emap[:n]], wd32[emap[:n]]),
        "lr swapped": _p_with(p, g, m, v, sumsq, Fc, lr32[swap][elem], wd32[elem]),
        "wd swapped": _p_with(p, g, m, v, sumsq, Fc, lr32[elem], wd32[swap][elem]),
        "group 0 everywhere": _p_with(p, g, m, v, sumsq, Fc, lr32[torch.zeros_like(elem)], wd32[torch.zeros_like(elem)]),
        "decay from base lr": _p_with(p, g, m, v, sumsq, Fc, lr32[elem], wd32[elem], decay_lr_e=torch.full((n,), f32eps(BASE_LR), dtype=torch.float64)),
    }
    out = []
    for label in MUTATIONS:
        mut = f64(got_p) + (wrong[label] - right)
        out.append((label, mut, orf.separated(mut, got_p, bound_p)))
    return out


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate_grouped(p, g, m, v, sumsq, Fc: dict, lr, wd, elem: torch.Tensor) -> Dict[str, np.ndarray]:
    """optimizer_reference.emulate_adamw (adamw_kernel operation by operation in fp32) per group"""
    n = p.numel()
    out = {k: np.zeros(n, dtype=np.float32) for k in ("p", "m", "v", "p_bf16", "g")}
    for k in sorted(set(elem.tolist())):
        idx = (elem == k).nonzero().flatten()
        r = orf.emulate_adamw(p[idx], g[idx], m[idx], v[idx], sumsq, dict(Fc, lr=f32eps(lr[k]), weight_decay=f32eps(wd[k])))
        for name in out:
            out[name][idx.numpy()] = r[name]
    return out
