"""fp64 references, per-element error bounds, inputs, mutations and an fp32 emulation for the optimiser pass of csrc/misc.hip:
wj_grad_sumsq, wj_adamw_step, wj_ema_update and wj_cast_f32_to_bf16 (test infrastructure; used by
tests/test_optimizer_reference_cpu.py and tests/test_optimizer_bounds_gpu.py).  The basics (U, KAPPA, bf16, bf16_bound, worst, check,
rejected, Guarded, f32eps) are those of tests/norm_reference.py.

Every reference function takes the inputs of one call as CPU tensors and the scalar fields AS THE FLOAT FIELDS THE KERNEL SEES
(`fields`), and returns {output: (fp64 reference, bound)}.  `check` requires every element finite and within its bound; no norms.

AdamW (the kernel's formula, which is torch.optim.AdamW behind clip_grad_norm_ applied to the SCALED gradient):
  norm = sqrt(sumsq) grad_scale        coef = grad_scale min(1, max_norm / (norm + 1e-6))     (no clip: coef = grad_scale)
  ge = g coef      pd = p (1 - lr wd)      m' = b1 m + (1 - b1) ge      v' = b2 v + (1 - b2) ge^2
  A = sqrt(v') / sqrt(bc2)      den = A + eps      upd = (lr / bc1) m' / den      p' = pd - upd
Bounds: first-order propagation through that arithmetic in fp32.  One rounding is w = 1.5 u, u = 2^-24 (norm_reference's 3 u for two
operations: a rounding is u of the COMPUTED value and reaches u of the reference at the bottom of a binade, so u itself leaves no
margin; a fused multiply-add rounds less often and stays inside).  sqrtf / rsqrtf / a division: FUN = 4 u each (two ulps: the
hardware's approximations are within one ulp, and one rounding).
  r_coef = 12 u where the clip is active (sqrt FUN, two products, one sum, a division FUN: 11 u, and the 1e-6 in fp32), else 0
  r_ge   = r_coef + w
  dm = w |b1 m| + (2 w + r_ge) |(1 - b1) ge| + w (|b1 m| + |(1 - b1) ge|)               (the only cancellation of m': the magnitudes)
  dv = w b2 v + (3 w + 2 r_ge) (1 - b2) ge^2 + w v'                                      (positive terms only)
  dpd = |pd| (w (1 + lr wd) / (1 - lr wd) + w)
  dA = A (dv / (2 v') + FUN + FUN + w)          (sqrtf, rsqrtf(bc2), their product; A = 0 where v' = 0)
  dden = dA + w den
  dupd = |upd| (FUN + w + FUN + dden / den) + (lr / bc1) dm / den                        (lr / bc1, the product, the division)
  dp = dpd + dupd + w (|pd| + |upd|)                                                     (the only cancellation of p')
  p_bf16: bit-equal to bf16 of the p the same launch wrote, and within bf16_bound(p', dp) of the reference.  g: unchanged, or exactly zero.
grad_sumsq: KAPPA u sum g^2, + u |result| for the final add of `accumulate`.
ema_update: t' = t r32 + (1 - r32) s (1 - r32 is exact in fp32 for r in [1/2, 1]): EMA_C u (|r t| + |q s|), EMA_C = 3: two products and
  one sum are 2 u (|r t| + |q s|) at worst; the third u is room for the reference program's coefficient float32(1 - r), which differs
  from 1 - r32 by up to 0.39 u |s| over the schedule r = 0.999 ... 0.99999.
cast: exact.

Mutations: a wrong formula evaluated in fp64 and applied as a delta to an accepted output (norm_reference._delta), or an edit of a
copy of it.  A mutation is CLAIMED on an input where the reference alone separates it: |mutated - accepted| > 2 bound on some element
(then no output within the bound of the reference can hide it).  REQUIRED names the (mutation, kind, state) triples that must be
claimed; the rest is claimed where it separates and never waived by hand.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.norm_reference import KAPPA, U, bf16, bf16_bound, f32eps, f64, mutate_truncate_bf16

FUN = 4.0                 # sqrtf, rsqrtf, a division: units of u
W = 1.5 * U               # one rounding
EMA_C = 3.0
CLIP_EPS = float(np.float32(1e-6))
F = np.float32

Pair = Tuple[torch.Tensor, torch.Tensor]

HANDLED = {
    "wj_adamw_args": {"p", "g", "m", "v", "p_bf16", "sumsq", "n", "lr", "beta1", "beta2", "eps", "weight_decay", "bc1", "bc2", "max_norm",
                      "grad_scale", "workgroups", "zero_grad"},
    "wj_sumsq_args": {"g", "out", "workspace", "n", "accumulate", "workgroups"},
    "wj_ema_args": {"student", "teacher", "teacher_bf16", "n", "r"},
    "wj_cast_args": {"src", "dst", "n"},
}
EXCLUDED: Dict[str, Dict[str, str]] = {}

KINDS = ("randn", "clipped", "scaled", "tiny", "zero", "mixed")
STATES = ("fresh", "warm")
WARM_STEPS = 100
HYPER = {
    "project": dict(lr=4e-4, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=0.04, max_norm=5.0),
    "nowd": dict(lr=1e-3, beta1=0.8, beta2=0.95, eps=1e-8, weight_decay=0.0, max_norm=1.0),
}
EMA_SCHEDULE = (0.999, 0.9995, 0.99999)


def fields(H: dict, step: int, grad_scale: float = 1.0, max_norm: Optional[float] = None) -> dict:
    """the float fields of wj_adamw_args as ops.adamw_step forms them from the hyper-parameters and the step number"""
    mx = H["max_norm"] if max_norm is None else max_norm
    return dict(lr=f32eps(H["lr"]), beta1=f32eps(H["beta1"]), beta2=f32eps(H["beta2"]), eps=f32eps(H["eps"]),
                weight_decay=f32eps(H["weight_decay"]), bc1=f32eps(1.0 - H["beta1"] ** step), bc2=f32eps(1.0 - H["beta2"] ** step),
                max_norm=f32eps(mx), grad_scale=f32eps(grad_scale))


# ------------------------------------------------------------------------------------------------------------ references
def grad_sumsq(g: torch.Tensor, out0=None, accumulate: bool = False) -> Dict[str, Pair]:
    s = (f64(g) ** 2).sum()
    o = f64(out0).reshape(()) if accumulate else torch.zeros((), dtype=torch.float64)
    ref = s + o
    bound = KAPPA * U * s + (U * ref.abs() if accumulate else 0.0)
    return {"out": (ref.reshape(1), bound.reshape(1))}


def _clip(sumsq, Fd: dict, how: str = "") -> Tuple[float, bool]:
    """(coef, the clip is active or near its threshold)"""
    gs = Fd["grad_scale"]
    if Fd["max_norm"] <= 0 or sumsq is None or how == "no_clip":
        return gs, False
    norm = float(f64(sumsq).reshape(-1)[0]) ** 0.5 * (1.0 if how == "clip_unscaled" else gs)
    ratio = Fd["max_norm"] / (norm + CLIP_EPS)
    return gs * min(1.0, ratio), ratio < 1.0 + 1e-5


def _adamw(p, g, m, v, sumsq, Fd: dict, how: str = "") -> dict:
    """the step in fp64; how: "" or the name of a wrong formula"""
    lr, b1, b2, eps, wd, bc1, bc2 = (Fd[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "bc1", "bc2"))
    coef, active = _clip(sumsq, Fd, how)
    ge = g * coef
    decay = 1.0 - lr * wd
    if how == "l2_wd":
        ge, decay = ge + wd * p, 1.0
    if how == "no_wd":
        decay = 1.0
    pd = p * decay
    bm = b2 if how == "beta2_in_m" else b1
    t1, t2 = bm * m, (1.0 - bm) * ge
    m1 = t1 + t2
    gv = g * Fd["grad_scale"] if how == "v_unclipped" else ge
    s1, s2 = b2 * v, (1.0 - b2) * gv * gv
    v1 = s1 + s2
    if how == "no_bc2":
        A = torch.sqrt(v1)
        den = A + eps
    elif how == "eps_in_sqrt":
        A = torch.sqrt(v1 / bc2)
        den = torch.sqrt(v1 / bc2 + eps * eps)
    elif how == "eps_before_bc2":
        A = torch.sqrt(v1) / bc2 ** 0.5
        den = (torch.sqrt(v1) + eps) / bc2 ** 0.5
    else:
        A = torch.sqrt(v1) / bc2 ** 0.5
        den = A + eps
    step = lr if how == "no_bc1" else lr / bc1
    upd = step * m1 / den
    return dict(p=pd - upd, m=m1, v=v1, pd=pd, upd=upd, t1=t1, t2=t2, s1=s1, s2=s2, A=A, den=den, step=step, active=active, decay=decay)


def adamw_step(p, g, m, v, sumsq, Fd: dict, zero_grad: bool = False) -> Dict[str, Pair]:
    """wj_adamw_step on one range: p, g, m, v f32 [n]; sumsq f32 [1] or None (no clipping)"""
    p, g, m, v = f64(p), f64(g), f64(m), f64(v)
    r = _adamw(p, g, m, v, sumsq, Fd)
    lr, wd = Fd["lr"], Fd["weight_decay"]
    r_ge = (12.0 * U if r["active"] else 0.0) + W
    t1, t2, s1, s2 = r["t1"].abs(), r["t2"].abs(), r["s1"], r["s2"]
    dm = W * t1 + (2 * W + r_ge) * t2 + W * (t1 + t2)
    dv = W * s1 + (3 * W + 2 * r_ge) * s2 + W * r["v"]
    dpd = r["pd"].abs() * (W * (1 + lr * wd) / r["decay"] + W)
    rel_v = torch.where(r["v"] > 0, dv / (2 * r["v"].clamp_min(1e-300)), torch.zeros_like(dv))
    dA = r["A"] * (rel_v + 2 * FUN * U + W)
    dden = dA + W * r["den"]
    dupd = r["upd"].abs() * (2 * FUN * U + W + dden / r["den"]) + r["step"] * dm / r["den"]
    dp = dpd + dupd + W * (r["pd"].abs() + r["upd"].abs())
    gout = torch.zeros_like(g) if zero_grad else g
    return {"p": (r["p"], dp), "m": (r["m"], dm), "v": (r["v"], dv), "p_bf16": (bf16(r["p"]), bf16_bound(r["p"], dp)),
            "g": (gout, torch.zeros_like(g))}


def ema_update(student, teacher, r: float) -> Dict[str, Pair]:
    s, t = f64(student), f64(teacher)
    r32 = f32eps(r)
    q = 1.0 - r32
    ref = t * r32 + q * s
    return {"teacher": (ref, EMA_C * U * ((r32 * t).abs() + (q * s).abs()))}


def ema_update_program(student, teacher, r: float) -> torch.Tensor:
    """the reference program's wording, teacher.mul_(r).add_((1 - r) student) with 1 - r formed in double and handed to fp32, in fp64"""
    return f64(teacher) * f32eps(r) + f32eps(1.0 - r) * f64(student)


def cast(src: torch.Tensor) -> torch.Tensor:
    return src.detach().cpu().float().to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------ inputs
def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def make_grad(kind: str, n: int, seed: int, H: dict, mag_seed: int = 0) -> Tuple[torch.Tensor, float]:
    """(g f32 [n], grad_scale).  The norms are set against max_norm, the tiny magnitude against eps."""
    x = torch.randn(n, generator=_gen(seed))
    mx, rn = H["max_norm"], float(n) ** 0.5
    if kind == "randn":             # ~ 1e-2, the norm at most 0.4 max_norm: clip inactive
        return x * min(1e-2, 0.4 * mx / rn), 1.0
    if kind == "clipped":           # norm ~ 10 max_norm
        return x * (10.0 * mx / rn), 1.0
    if kind == "scaled":            # norm ~ 16 max_norm, scaled ~ 2 max_norm: coef = grad_scale / 2, from the unscaled norm grad_scale / 16
        return x * (16.0 * mx / rn), 0.125
    if kind == "tiny":              # sqrt(v) at or below eps
        return x * (0.1 * H["eps"]), 1.0
    if kind == "zero":
        return torch.zeros(n), 1.0
    if kind == "mixed":             # twelve decades of magnitude, fixed per element; the sign is drawn per call
        mag = 10.0 ** (-12.0 * torch.rand(n, generator=_gen(mag_seed + 7919), dtype=torch.float64))
        return (torch.sign(x).double() * mag).float(), 1.0
    raise ValueError(kind)


@functools.lru_cache(maxsize=64)
def _warm_state(kind: str, n: int, hyper: str, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """m, v after WARM_STEPS fp64 steps on independent gradients of the kind, rounded to f32"""
    H = HYPER[hyper]
    m = torch.zeros(n, dtype=torch.float64)
    v = torch.zeros(n, dtype=torch.float64)
    for k in range(1, WARM_STEPS + 1):
        g, gs = make_grad(kind, n, seed + 1000 + k, H, mag_seed=seed)
        g = g.double()
        coef, _ = _clip((g * g).sum(), fields(H, k, gs))
        ge = g * coef
        m.mul_(H["beta1"]).add_(ge, alpha=1.0 - H["beta1"])
        v.mul_(H["beta2"]).addcmul_(ge, ge, value=1.0 - H["beta2"])
    return m.float(), v.float()


def adamw_case(kind: str, state: str, n: int, hyper: str, seed: int) -> dict:
    """p, g, m, v f32 [n] (fresh copies), step, grad_scale, the hyper-parameters.  mixed + warm: m and ge differ in sign on about half of
    the elements (the sign of g is drawn per step)."""
    H = HYPER[hyper]
    g, gs = make_grad(kind, n, seed, H, mag_seed=seed)
    p = torch.randn(n, generator=_gen(seed + 1))
    if state == "fresh":
        m, v, step = torch.zeros(n), torch.zeros(n), 1
    else:
        m, v = (t.clone() for t in _warm_state(kind, n, hyper, seed))
        step = WARM_STEPS + 1
    return dict(p=p, g=g, m=m, v=v, step=step, grad_scale=gs, H=H, kind=kind, state=state, hyper=hyper)


def ema_case(n: int, seed: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """student and teacher with |s| ~ |t| element by element (the teacher is the student's own moving average: 5 % apart)"""
    s = torch.randn(n, generator=_gen(seed))
    return s, (s * (1 + 0.05 * torch.randn(n, generator=_gen(seed + 1)))).contiguous()


# ------------------------------------------------------------------------------------------------------------ mutations
FORMULAS = ("no_bc2", "no_bc1", "eps_in_sqrt", "eps_before_bc2", "no_clip", "clip_unscaled", "v_unclipped", "beta2_in_m", "no_wd", "l2_wd")
_LIVE = ("randn", "clipped", "scaled", "mixed")
# (mutation, output) -> the (kind, state) pairs on which it must be claimed; "wd": only with weight decay
REQUIRED = {
    ("no_bc2", "p"): {(k, s) for k in _LIVE for s in STATES},
    ("no_bc1", "p"): {(k, "fresh") for k in _LIVE + ("tiny",)},
    ("eps_in_sqrt", "p"): {("tiny", s) for s in STATES},
    ("eps_before_bc2", "p"): {("tiny", s) for s in STATES},
    # (from m = v = 0 the update is lr sign(g) |ge| / (|ge| + eps sqrt(bc2) / ...): the first step does not see the scale of the gradient
    #  in p, only in m and v)
    ("no_clip", "p"): {("clipped", "warm")},
    ("no_clip", "m"): {("clipped", s) for s in STATES},
    ("clip_unscaled", "p"): {("scaled", "warm")},
    ("clip_unscaled", "m"): {("scaled", s) for s in STATES},
    ("clip_unscaled", "v"): {("scaled", s) for s in STATES},
    ("v_unclipped", "v"): {("clipped", s) for s in STATES},
    ("beta2_in_m", "m"): {(k, s) for k in _LIVE + ("tiny",) for s in STATES},
    ("no_wd", "p"): {(k, s) for k in KINDS for s in STATES},
    ("l2_wd", "p"): {(k, s) for k in KINDS for s in STATES},
    ("stale vector", "p"): {(k, s) for k in _LIVE for s in STATES},
    ("stale vector", "m"): {(k, s) for k in _LIVE for s in STATES},
    ("stale vector", "v"): {(k, s) for k in _LIVE for s in STATES},
    ("vectors swapped", "p"): {(k, s) for k in KINDS for s in STATES},
    ("vectors swapped", "m"): {(k, s) for k in _LIVE for s in STATES},
    ("vectors swapped", "v"): {(k, s) for k in _LIVE for s in STATES},
    ("bf16 truncated", "p_bf16"): {(k, s) for k in KINDS for s in STATES},
}
NEEDS_WD = {"no_wd", "l2_wd"}


def separated(mut: torch.Tensor, got: torch.Tensor, bound: torch.Tensor) -> bool:
    """the reference alone separates the mutation: it moves some element of an accepted output by more than twice its bound"""
    d = (f64(mut) - f64(got)).abs()
    return bool((~torch.isfinite(d)).any()) or bool((d > 2 * bound).any())


def adamw_mutations(c: dict, sumsq, Fd: dict, got: Dict[str, torch.Tensor], ref: Dict[str, Pair]) -> List[tuple]:
    """[(label, output, mutated, claimed)] of the outputs `got` ({p, m, v, p_bf16}: CPU tensors of one accepted launch on the case c).
    Needs n >= 12."""
    p, g, m, v = (f64(c[k]) for k in ("p", "g", "m", "v"))
    right = _adamw(p, g, m, v, sumsq, Fd)
    out = []
    for how in FORMULAS:
        wrong = _adamw(p, g, m, v, sumsq, Fd, how)
        for k in ("p", "m", "v"):
            mut = f64(got[k]) + (wrong[k] - right[k])
            out.append((how, k, mut, separated(mut, got[k], ref[k][1])))
    for k in ("p", "m", "v"):
        stale = f64(got[k]).clone()
        stale[4:8] = f64(c[k])[4:8]
        out.append(("stale vector", k, stale, separated(stale, got[k], ref[k][1])))
        sw = f64(got[k]).clone()
        sw[4:8], sw[8:12] = f64(got[k])[8:12], f64(got[k])[4:8]
        out.append(("vectors swapped", k, sw, separated(sw, got[k], ref[k][1])))
    # a whole ulp off on about half of the elements against a bound of half an ulp: always claimed
    out.append(("bf16 truncated", "p_bf16", mutate_truncate_bf16(got["p"]), True))
    return out


def required_missing(c: dict, muts: List[tuple]) -> List[str]:
    """the REQUIRED triples of this case that the mutation list does not claim"""
    claimed = {(label, k) for label, k, _, cl in muts if cl}
    miss = []
    for (label, k), pairs in REQUIRED.items():
        if label in NEEDS_WD and c["H"]["weight_decay"] == 0:
            continue
        if (c["kind"], c["state"]) in pairs and (label, k) not in claimed:
            miss.append(f"{label} ({k}) on {c['kind']} / {c['state']} / {c['hyper']}")
    return miss


def mutate_sumsq_drop_last(got, g) -> torch.Tensor:
    """the last 4-element vector left out of the sum"""
    return f64(got) - (f64(g)[-4:] ** 2).sum()


def sumsq_last_vector_separates(g) -> bool:
    """4 g^2 against KAPPA u sum g^2: the last vector's squares exceed twice the bound"""
    s = (f64(g) ** 2).sum()
    return bool((f64(g)[-4:] ** 2).sum() > 2 * (KAPPA * U * s + U * s))


def mutate_sumsq_ignore_out0(got, out0) -> torch.Tensor:
    return f64(got) - f64(out0).reshape(-1)[0]


def mutate_ema_exchanged(got, student, teacher, r: float) -> torch.Tensor:
    """r and 1 - r exchanged"""
    s, t, r32 = f64(student), f64(teacher), f32eps(r)
    return f64(got) + ((1.0 - r32) * t + r32 * s) - (r32 * t + (1.0 - r32) * s)


def mutate_ema_neighbour(got, student, teacher, r: float) -> torch.Tensor:
    """element i reads the teacher at i + 1 (the last one its own)"""
    t, r32 = f64(teacher), f32eps(r)
    tn = torch.cat([t[1:], t[-1:]])
    return f64(got) + r32 * (tn - t)


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def _rsqrt(x):
    return F(1.0 / np.sqrt(np.float64(x)))


def emulate_adamw(p, g, m, v, sumsq, Fd: dict) -> Dict[str, np.ndarray]:
    """adamw_kernel, operation by operation in fp32 (no fused multiply-add)"""
    p, g, m, v = (t.detach().cpu().numpy().astype(F) for t in (p, g, m, v))
    lr, b1, b2, eps, wd, bc1, bc2, mx, gs = (F(Fd[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "bc1", "bc2", "max_norm", "grad_scale"))
    coef = gs
    if mx > 0 and sumsq is not None:
        norm = F(np.sqrt(F(float(sumsq.reshape(-1)[0]))) * gs)
        coef = F(coef * np.minimum(F(1.0), F(mx / F(norm + F(1e-6)))))
    decay = F(F(1.0) - F(lr * wd))
    step = F(lr / bc1)
    rbc2 = _rsqrt(bc2)
    ge = (g * coef).astype(F)
    p = (p * decay).astype(F)
    m = ((b1 * m).astype(F) + (F(F(1.0) - b1) * ge).astype(F)).astype(F)
    v = ((b2 * v).astype(F) + ((F(F(1.0) - b2) * ge).astype(F) * ge).astype(F)).astype(F)
    den = ((np.sqrt(v).astype(F) * rbc2).astype(F) + eps).astype(F)
    p = (p - ((step * m).astype(F) / den).astype(F)).astype(F)
    return {"p": p, "m": m, "v": v, "p_bf16": torch.from_numpy(p).to(torch.bfloat16).float().numpy(), "g": g}


def emulate_ema(student, teacher, r: float) -> np.ndarray:
    s, t = student.numpy().astype(F), teacher.numpy().astype(F)
    r32 = F(r)
    q = F(F(1.0) - r32)
    return ((t * r32).astype(F) + (q * s).astype(F)).astype(F)


def emulate_ema_program(student, teacher, r: float) -> np.ndarray:
    s, t = student.numpy().astype(F), teacher.numpy().astype(F)
    return ((t * F(r)).astype(F) + (F(1.0 - r) * s).astype(F)).astype(F)


def _butterfly(v: np.ndarray) -> np.ndarray:
    L = v.shape[-1]
    idx = np.arange(L)
    o = L // 2
    while o > 0:
        v = (v + v[..., idx ^ o]).astype(F)
        o >>= 1
    return v[..., 0]


def _block_sum(acc: np.ndarray) -> np.ndarray:
    """[blocks][threads] -> [blocks]: wave butterflies, then the waves in order"""
    waves = _butterfly(acc.reshape(acc.shape[0], -1, 64))
    tot = np.zeros(acc.shape[0], dtype=F)
    for w in range(waves.shape[1]):
        tot = (tot + waves[:, w]).astype(F)
    return tot


def sumsq_grid(n: int, workgroups: int = 0) -> int:
    grid = max(1, min(1024, (n // 4 + 255) // 256))
    return workgroups if 0 < workgroups < grid else grid


def emulate_sumsq(g, out0=None, accumulate: bool = False, workgroups: int = 0) -> np.ndarray:
    """a lane's strided chain of ((a^2 + b^2) + c^2) + d^2, block_sum of 256, then the 1024-thread fold of the workgroups' partials"""
    x = g.detach().cpu().numpy().astype(F)
    n4 = x.shape[0] // 4
    grid = sumsq_grid(x.shape[0], workgroups)
    T = grid * 256
    it = -(-n4 // T)
    pad = np.zeros((it * T, 4), dtype=F)
    pad[:n4] = x[:n4 * 4].reshape(n4, 4)
    sq = (pad * pad).astype(F).reshape(it, T, 4)
    acc = np.zeros(T, dtype=F)
    for i in range(it):
        q = (((sq[i, :, 0] + sq[i, :, 1]).astype(F) + sq[i, :, 2]).astype(F) + sq[i, :, 3]).astype(F)
        acc = (acc + q).astype(F)
    ws = _block_sum(acc.reshape(grid, 256))
    fin = np.zeros(1024, dtype=F)
    fin[:grid] = ws
    s = _block_sum(fin.reshape(1, 1024))[0]
    if accumulate:
        s = F(F(float(out0.reshape(-1)[0])) + s)
    return np.array([s], dtype=F)
