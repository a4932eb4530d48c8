"""fp64 references, per-element error bounds, guard rows and mutations for the LayerNorm family, the column sums, the teacher targets
and the masked MSE (test infrastructure; used by tests/test_norm_reference_cpu.py and tests/test_norm_bounds_gpu.py).

Every reference function takes the inputs of one call as CPU tensors and returns {output: (fp64 reference, bound)}: the reference at
the rounding points include/wavjepa_hip.h documents (s = fl32(x + r), y_bf16 = bf16(y), ...), the bound with the shape of the output.
`check` requires every element finite and within its bound; there is no norm anywhere.  The mutation helpers edit a copy of a correct
output the way a subtly wrong kernel would; `check` must reject each of them.  The `emulate_*` functions redo the arithmetic in fp32
numpy in the order the kernels document (a lane's own <= 16 elements, then a butterfly over the lanes of the row); they measure the
margin of the bounds on the reference side only.

Bounds: first-order propagation through the documented arithmetic, u = 2^-24, one summation constant KAPPA.
LayerNorm forward, c = s - mu, A = mean|s|, xh = c rstd:
  dmu = KAPPA u A                          dc = u |c| + dmu
  dvar = KAPPA u var + 2 dmu mean|c| + dmu^2
  drstd / rstd = KAPPA u + dvar / (2 (var + eps))
  dxh = rstd dc + |xh| drstd / rstd        dy = |gamma| dxh + 3 u (|gamma xh| + |beta|)
  mean: dmu + u |mu|;  rstd: rstd (drstd / rstd + u);  bf16 outputs: e (1 + 2^-8) + 2^-8 |ref| (+ a straddled rounding boundary: bf16_bound).
LayerNorm backward, g = dy gamma, k1 = mean g, k2 = mean g xh, ds = rstd (g - k1 - xh k2): xh carries dxh with the bound of the STORED
mean and rstd; dk1 = KAPPA u mean|g|; dk2 = KAPPA u mean|g xh| + mean(|g| dxh); the rest term by term.
Column quantities: KAPPA u sum_rows |term| (+ the propagated per-term error).  dbias is defined on the bf16 ds the launch wrote.
instnorm_mean: the one-pass variance carries kappa = (s2 / n) / (var + eps): dvar = 2 KAPPA u kappa (var + eps).
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

U = 2.0 ** -24
KAPPA = 8.0
BF16_ROUND = 2.0 ** -8
GUARD = 3                 # NaN rows in front of and behind every guarded output
SPLIT = 4                 # WJ_GROUP_STATS_SPLIT

Pair = Tuple[torch.Tensor, torch.Tensor]

# Fields of the argument structs the references understand (operands, outputs, shapes and switches), and the ones left to other tests.
# tests/test_norm_reference_cpu.py holds the header against these lists: a field added later fails there.
HANDLED = {
    "wj_ln_fwd_args": {"x", "r", "gamma", "beta", "y_f32", "y_bf16", "mean", "rstd", "group_stats", "M", "D", "x_is_bf16", "in_seg",
                       "in_valid", "group_rows", "in_chan", "eps"},
    "wj_ln_bwd_args": {"dy", "dy2", "x", "r", "gamma", "mean", "rstd", "ds_f32", "ds_bf16", "dgamma", "dbeta", "dbias", "workspace", "M", "D",
                       "x_is_bf16", "in_seg", "in_valid", "out_seg", "out_valid", "chan", "dy2_is_bf16"},
    "wj_ln_pre_fwd_args": {"x", "r", "gamma", "beta", "s_f32", "y_f32", "y_bf16", "mean", "rstd", "group_stats", "M", "D", "group_rows", "eps"},
    "wj_ln_pre_bwd_args": {"dy", "dres", "s", "gamma", "mean", "rstd", "ds_f32", "ds_bf16", "dgamma", "dbeta", "dbias", "workspace", "M", "D",
                           "dy_is_bf16"},
    "wj_colsum_args": {"x", "out", "ldx", "M", "N", "workspace", "workspace_bytes", "deterministic"},
    "wj_colsum_group_args": {"x", "o0", "o1", "o2", "ldx", "M", "N", "n_each", "n", "deterministic"},
    "wj_instnorm_args": {"x", "targets", "B", "TD", "accumulate", "scale", "eps"},
    "wj_instnorm_mean_args": {"x0", "x1", "x2", "x3", "x4", "x5", "x6", "x7", "stats", "targets", "B", "TD", "K", "eps"},
    "wj_mse_args": {"preds", "targets", "tgt", "rows", "loss", "dpreds", "workspace", "gscale_ptr", "B", "G", "T", "D", "n_rows", "gscale"},
}
EXCLUDED = {
    "wj_ln_fwd_args": {"y_fp8": "test_fp8_outputs_fused_into_layernorm_and_gelu_epilogue",
                       "y_fp8_scales": "test_fp8_outputs_fused_into_layernorm_and_gelu_epilogue",
                       "ld_fp8_scale": "test_fp8_outputs_fused_into_layernorm_and_gelu_epilogue",
                       "workgroups": "the lean form is held bit-identical to the full form by test_layernorm_fwd_lean_form_on_a_capped_grid"},
}

KINDS = ("randn", "offset", "outlier", "tiny", "constant", "zero")
WIDTHS = (4, 36, 128, 200, 260, 384, 516, 640, 768, 772, 1000, 1024)


# ------------------------------------------------------------------------------------------------------------ basics
def f64(t) -> torch.Tensor:
    return t.detach().to("cpu").double()


def f32eps(eps: float) -> float:
    """eps as the kernels see it (a float field of the argument struct)"""
    return float(np.float32(eps))


def bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.bfloat16).double()


def bf16_bound(v: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """Bound of a bf16 output whose value in front of the rounding is v, known to within e: the rule of tests/gemm_reference.py,
    e (1 + 2^-8) + 2^-8 |ref|, plus one term.  2^-8 |ref| is half an ulp at the bottom of a binade, and a correct kernel whose value lies
    within e of a rounding boundary lands a whole ulp from ref = bf16(v) however small e is (rounding is monotone: the output lies in
    [bf16(v - e), bf16(v + e)]).  The width of that interval is added: zero wherever no boundary lies within e of v, so that everywhere
    else the rule stands as it is -- a truncating conversion is a whole ulp off on half of the elements."""
    ref = bf16(v)
    return e * (1 + BF16_ROUND) + BF16_ROUND * ref.abs() + (bf16(v + e) - bf16(v - e)).abs()


def add_f32(x: torch.Tensor, r: Optional[torch.Tensor]) -> torch.Tensor:
    """s = fl32(x + r): the row that is normalised, as fp64 (x f32 or bf16, r bf16 or None)"""
    s = x.detach().cpu().float()
    if r is not None:
        s = s + r.detach().cpu().float()
    return s.double()


def worst(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of |got - ref| / bound (0 / 0 = 0); inf when an element is not finite or off where the bound is zero"""
    got = f64(got)
    if got.shape != ref.shape:
        got = got.reshape(ref.shape)
    if got.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(ratio.max())


def where_worst(got, ref, bound) -> str:
    got = f64(got).reshape(ref.shape)
    bad = ~torch.isfinite(got)
    err = torch.where(bad, torch.full_like(ref, float("inf")), (got - ref).abs())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    i = int(ratio.flatten().argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape))) if ref.dim() else ()
    return f"at {idx}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bound {float(bound.flatten()[i]):.3e}"


def check(got, ref: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """Every element finite and within its bound.  Returns the worst error / bound."""
    w = worst(got, ref, bound)
    assert w <= 1.0, f"{what}: error / bound = {w:.3g} {where_worst(got, ref, bound)}"
    return w


def rejected(got, ref, bound) -> bool:
    return worst(got, ref, bound) > 1.0


class Guarded:
    """An [M][*] output between GUARD rows, all NaN before the launch: a kernel must overwrite all of [M][D] and nothing else."""
    def __init__(self, M: int, D: Optional[int] = None, dtype=torch.float32, device="cpu"):
        shape = (M + 2 * GUARD,) + ((D,) if D else ())
        self.buf = torch.full(shape, float("nan"), dtype=dtype, device=device)
        self.view = self.buf[GUARD:GUARD + M]

    def guards_intact(self) -> bool:
        n = self.view.shape[0]
        return bool(torch.isnan(self.buf[:GUARD].float()).all()) and bool(torch.isnan(self.buf[GUARD + n:].float()).all())

    def check(self, what: str) -> torch.Tensor:
        assert self.guards_intact(), f"{what}: a guard row was written"
        return self.view


def guarded_like(M: int, D: Optional[int], dtype, device, fill: Optional[torch.Tensor] = None) -> Guarded:
    g = Guarded(M, D, dtype, device)
    if fill is not None:
        g.view.copy_(fill)
    return g


# ------------------------------------------------------------------------------------------------------------ inputs
def make_rows(kind: str, M: int, D: int, seed: int) -> torch.Tensor:
    """[M][D] f32 of one input kind (the row s that is normalised, before the optional bf16 addend)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, D, generator=g)
    if kind == "randn":
        return x
    if kind == "offset":
        return x + 1000.0
    if kind == "outlier":
        x[:, (D // 2) | 1 if D > 1 else 0] *= 1e4
        return x
    if kind == "tiny":
        return x * 1e-4
    if kind == "constant":
        return x[:, :1].expand(M, D).contiguous()
    if kind == "zero":
        return torch.zeros(M, D)
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
def _row_stats(s: torch.Tensor, eps: float) -> dict:
    mu = s.mean(1, keepdim=True)
    c = s - mu
    var = (c * c).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    dmu = KAPPA * U * s.abs().mean(1, keepdim=True)
    dc = U * c.abs() + dmu
    dvar = KAPPA * U * var + 2 * dmu * c.abs().mean(1, keepdim=True) + dmu * dmu
    drel = KAPPA * U + dvar / (2 * (var + eps))
    xh = c * rstd
    return dict(mu=mu, c=c, var=var, rstd=rstd, xh=xh, dmu=dmu, dc=dc, dvar=dvar, drel=drel, dxh=rstd * dc + xh.abs() * drel,
                b_mean=dmu + U * mu.abs(), b_rstd=rstd * (drel + U))


def layernorm_fwd(x, r, gamma, beta, eps: float) -> Dict[str, Pair]:
    """wj_layernorm_fwd: x [M][D] f32 or bf16 ALREADY gathered through the row remap, r bf16 or None."""
    s = add_f32(x, r)
    eps = f32eps(eps)
    gamma, beta = f64(gamma), f64(beta)
    st = _row_stats(s, eps)
    y = st["xh"] * gamma + beta
    dy = gamma.abs() * st["dxh"] + 3 * U * ((gamma * st["xh"]).abs() + beta.abs())
    yb = bf16(y)
    return {"s_f32": (s, torch.zeros_like(s)), "y_f32": (y, dy), "y_bf16": (yb, bf16_bound(y, dy)),
            "mean": (st["mu"][:, 0], st["b_mean"][:, 0]), "rstd": (st["rstd"][:, 0], st["b_rstd"][:, 0])}


def layernorm_pre_fwd(x, r, gamma, beta, eps: float) -> Dict[str, Pair]:
    """wj_layernorm_pre_fwd: the same arithmetic; s_f32 is an output (bit-exact fl32(x + r): its bound is zero)."""
    return layernorm_fwd(x, r, gamma, beta, eps)


def group_stats(v: torch.Tensor, dv: Optional[torch.Tensor], group_rows: int) -> Dict[str, Pair]:
    """(sum v, sum v^2) per group of group_rows rows and quarter of the group, [G][SPLIT][2], and the group totals [G][2] (the quarters
    added in fp64).  v: fp64 [M][D] (y of the post-norm forward with its bound dv, the stream s of the pre-norm one with dv = None)."""
    M = v.shape[0]
    G = -(-M // group_rows)
    rpp = -(-group_rows // SPLIT)
    ref = torch.zeros(G, SPLIT, 2, dtype=torch.float64)
    bnd = torch.zeros(G, SPLIT, 2, dtype=torch.float64)
    dv = torch.zeros_like(v) if dv is None else dv
    for g in range(G):
        for q in range(SPLIT):
            lo, hi = g * group_rows + q * rpp, min(M, g * group_rows + min(group_rows, (q + 1) * rpp))
            if lo >= hi:
                continue
            b, db = v[lo:hi], dv[lo:hi]
            ref[g, q, 0], ref[g, q, 1] = b.sum(), (b * b).sum()
            bnd[g, q, 0] = KAPPA * U * b.abs().sum() + db.sum()
            bnd[g, q, 1] = KAPPA * U * (b * b).sum() + (2 * b.abs() * db + db * db).sum()
    return {"parts": (ref, bnd), "total": (ref.sum(1), bnd.sum(1))}


def _ln_bwd(s, dy, gamma, eps, dres) -> Dict[str, Pair]:
    st = _row_stats(s, eps)
    xh, rstd = st["xh"], st["rstd"]
    # x-hat from the STORED mean and rstd (each within its forward bound), one subtraction and one product
    dxh = rstd * (U * st["c"].abs() + st["b_mean"]) + xh.abs() * (st["b_rstd"] / rstd + 2 * U)
    g = dy * gamma
    k1 = g.mean(1, keepdim=True)
    k2 = (g * xh).mean(1, keepdim=True)
    dk1 = (KAPPA + 1) * U * g.abs().mean(1, keepdim=True)
    dk2 = (KAPPA + 2) * U * (g * xh).abs().mean(1, keepdim=True) + (g.abs() * dxh).mean(1, keepdim=True)
    t = g - k1 - xh * k2
    dt = U * g.abs() + dk1 + dxh * k2.abs() + xh.abs() * dk2 + 3 * U * (g.abs() + k1.abs() + (xh * k2).abs())
    ds = rstd * t
    dds = rstd * dt + ds.abs() * (st["b_rstd"] / rstd + U)
    if dres is not None:
        ds = ds + dres
        dds = dds + 2 * U * ds.abs()       # one addition; u alone is attained at the bottom of a binade (the forward's 3 u is for two operations)
    dsb = bf16(ds)
    dgamma = (dy * xh).sum(0)
    b_dgamma = KAPPA * U * (dy * xh).abs().sum(0) + (dy.abs() * dxh).sum(0) + U * (dy * xh).abs().sum(0)
    return {"ds_f32": (ds, dds), "ds_bf16": (dsb, bf16_bound(ds, dds)), "dgamma": (dgamma, b_dgamma),
            "dbeta": (dy.sum(0), KAPPA * U * dy.abs().sum(0)), "_terms": (dy * xh, dy)}


def layernorm_bwd(dy, dy2, x, r, gamma, eps: float) -> Dict[str, Pair]:
    """wj_layernorm_bwd: dy f32 (+ dy2 f32 or bf16, added in fp32), x (+ r) as the forward; mean and rstd are the forward's (the bound
    carries their forward bounds).  dgamma / dbeta are the sums alone: add what the buffers held before."""
    d = dy.detach().cpu().float()
    if dy2 is not None:
        d = d + dy2.detach().cpu().float()
    return _ln_bwd(add_f32(x, r), d.double(), f64(gamma), f32eps(eps), None)


def layernorm_pre_bwd(dy, dres, s, gamma, eps: float) -> Dict[str, Pair]:
    """wj_layernorm_pre_bwd: ds = (dres) + LN-backward(dy; s); dy f32 or bf16."""
    return _ln_bwd(f64(s), f64(dy), f64(gamma), f32eps(eps), None if dres is None else f64(dres))


def dbias(ds_bf16_got: torch.Tensor) -> Pair:
    """dbias is DEFINED as the column sum of the bf16 ds the same launch wrote ([M][D], padding rows excluded)"""
    d = f64(ds_bf16_got)
    return d.sum(0), KAPPA * U * d.abs().sum(0)


# ------------------------------------------------------------------------------------------------------------ column sums
def colsum(x: torch.Tensor, out0: Optional[torch.Tensor] = None) -> Pair:
    """out0 + column sums of x [M][N] (f32 or bf16; the caller slices ldx away): wj_colsum_f32 / wj_colsum_bf16"""
    x = f64(x)
    o = torch.zeros(x.shape[1], dtype=torch.float64) if out0 is None else f64(out0)
    return o + x.sum(0), KAPPA * U * (x.abs().sum(0) + o.abs())


colsum_f32 = colsum
colsum_bf16 = colsum


def colsum_f32_group(x: torch.Tensor, n_each: int, outs0: List[Optional[torch.Tensor]]) -> List[Optional[Pair]]:
    """one item of wj_colsum_f32_group: columns [0, n_each) -> o0, [n_each, 2 n_each) -> o1, the rest -> o2; None outputs stay None"""
    N = x.shape[1]
    res: List[Optional[Pair]] = []
    for w, o in enumerate(outs0):
        lo, hi = min(N, w * n_each), min(N, (w + 1) * n_each) if w < 2 else N
        if o is None:
            res.append(None)
            continue
        ref, bnd = f64(o).clone(), KAPPA * U * f64(o).abs()
        r, b = colsum(x[:, lo:hi])
        ref[:hi - lo] += r
        bnd[:hi - lo] += b
        res.append((ref, bnd))
    return res


# ------------------------------------------------------------------------------------------------------------ teacher targets
def instnorm_accumulate(x, prev, scale: float, eps: float) -> Dict[str, Pair]:
    """wj_instnorm_accumulate: x [B][TD]; targets = (prev +) (x - mean) rsqrt(var + eps) scale, two-pass statistics"""
    x = f64(x)
    st = _row_stats(x, f32eps(eps))
    scale = float(np.float32(scale))
    k = st["rstd"] * scale
    t = st["c"] * k
    dt = abs(scale) * st["dxh"] + 2 * U * t.abs()
    if prev is not None:
        t = t + f64(prev)
        dt = dt + U * t.abs()
    return {"targets": (t, dt)}


def instnorm_mean(xs, eps: float) -> Dict[str, Pair]:
    """wj_instnorm_mean: xs K tensors [B][TD]; targets = (1/K) sum_l instance-norm(x_l).  The kernel forms var = s2/n - mu^2 from fp32
    sums: the bound carries kappa = (s2/n) / (var + eps), returned as "kappa" [K][B] (bound slot: zeros)."""
    eps = f32eps(eps)
    K = len(xs)
    out, bnd, mag, kap = 0.0, 0.0, 0.0, []
    for x in xs:
        x = f64(x)
        mu = x.mean(1, keepdim=True)
        c = x - mu
        var = (c * c).mean(1, keepdim=True)
        s2n = (x * x).mean(1, keepdim=True)
        kappa = s2n / (var + eps)
        rstd = 1.0 / torch.sqrt(var + eps)
        dmu = KAPPA * U * x.abs().mean(1, keepdim=True)
        dvar = 2 * KAPPA * U * kappa * (var + eps)
        drel = KAPPA * U + dvar / (2 * (var + eps))
        t = c * rstd / K
        dt = (rstd * (U * c.abs() + dmu) + (c * rstd).abs() * drel) / K + 3 * U * t.abs()
        out, bnd, mag = out + t, bnd + dt, mag + t.abs()
        kap.append(kappa[:, 0])
    kap = torch.stack(kap)
    return {"targets": (out, bnd + K * U * mag), "kappa": (kap, torch.zeros_like(kap))}


# ------------------------------------------------------------------------------------------------------------ masked MSE
def masked_mse(preds, targets, tgt, B: int, G: int, T: int, D: int, gscale: float = 1.0, gscale_dev: Optional[float] = None,
               rows: Optional[torch.Tensor] = None) -> Dict[str, Pair]:
    """wj_masked_mse: preds bf16 [R][D] (R = B G T, or the listed rows of the ragged form), targets f32 [B][T][D], tgt u8 [B][G][T]
    (any non-zero byte is a target).  loss[1] = count is exact; dpreds is exactly zero on rows that are not targets."""
    p = f64(preds).reshape(-1, D)
    y = f64(targets).reshape(B, T, D)
    on_dense = (tgt.detach().cpu().reshape(-1) != 0)
    dense = torch.arange(B * G * T) if rows is None else rows.detach().cpu().long()
    R = dense.numel()
    p = p[:R]
    count = float(on_dense.sum())
    den = count + float(np.float32(1e-8))
    on = on_dense[dense].double()[:, None]
    b, t = (dense // T) // G, dense % T
    d = (p - y[b, t]) * on
    err = (d * d).mean(1)
    derr = (KAPPA + 4) * U * err
    loss0 = err.sum() / den
    b0 = (KAPPA * U * err.abs().sum() + derr.sum()) / den + 2 * U * abs(loss0)
    gk = 2.0 / (D * den) * float(np.float32(gscale)) * (1.0 if gscale_dev is None else float(np.float32(gscale_dev)))
    v = d * gk
    vb = bf16(v)
    return {"loss": (torch.stack([loss0, torch.tensor(count, dtype=torch.float64)]), torch.stack([b0, torch.tensor(0.0, dtype=torch.float64)])),
            "dpreds": (vb, bf16_bound(v, 6 * U * v.abs()) * on), "_on": (on[:, 0], on[:, 0])}


# ------------------------------------------------------------------------------------------------------------ mutations
# Each takes a correct output (a CPU tensor, any float dtype) and what it needs of the inputs, and returns an edited fp64 copy.
def _delta(got, ref_right, ref_wrong):
    """a correct output moved by the difference between the wrong and the right formula"""
    return f64(got) + (ref_wrong - ref_right)


def _ln_y(s, gamma, beta, var_of: Callable, eps) -> Tuple[torch.Tensor, torch.Tensor]:
    mu = s.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var_of(s, mu) + eps)
    return (s - mu) * rstd * gamma + beta, rstd[:, 0]


def _var(s, mu):
    return ((s - mu) ** 2).mean(1, keepdim=True)


def mutate_ln_variance(got_y, got_rstd, s, gamma, beta, eps: float, how: str):
    """how: "dm1" (variance over D - 1), "no_eps", "one_pass" (E[s^2] - mu^2 in fp32).  Returns (y, rstd)."""
    s, gamma, beta, eps = f64(s), f64(gamma), f64(beta), f32eps(eps)
    D = s.shape[1]
    y0, r0 = _ln_y(s, gamma, beta, _var, eps)
    if how == "dm1":
        y1, r1 = _ln_y(s, gamma, beta, lambda s_, mu: _var(s_, mu) * D / max(D - 1, 1), eps)
    elif how == "no_eps":
        y1, r1 = _ln_y(s, gamma, beta, _var, 1e-30)
    elif how == "one_pass":
        def one_pass(s_, mu):
            s32 = s_.float()
            m32 = s32.mean(1, keepdim=True)
            return ((s32 * s32).mean(1, keepdim=True) - m32 * m32).clamp_min(0).double()
        y1, r1 = _ln_y(s, gamma, beta, one_pass, eps)
    else:
        raise ValueError(how)
    return _delta(got_y, y0, y1), _delta(got_rstd, r0, r1)


def mutate_chunk(got, row: int, chunk: int, value: float = 0.0):
    """one float4 chunk of one row left zero (or, value = nan, unwritten)"""
    m = f64(got).clone()
    m[row, 4 * chunk:4 * chunk + 4] = value
    return m


def mutate_swap_rows(got, row: int):
    m = f64(got).clone()
    m[[row, row + 1]] = m[[row + 1, row]]
    return m


def mutate_colsum_row(got, term_row, sign: float):
    """sign = -1: a row missing from a column sum; +1: a row counted twice (also: the re-read row of a dead second slot added in)"""
    return f64(got) + sign * f64(term_row)


def mutate_truncate_bf16(got_f32):
    """bf16 by truncation instead of round-to-nearest-even, from the f32 output of the same launch"""
    bits = got_f32.detach().cpu().float().contiguous().view(torch.int32)
    return (bits & -65536).view(torch.float32).double()


def mutate_route(o0_got, o1_got, colsum_last: float):
    """the last column of o0 routed to the neighbouring output at the n_each boundary"""
    a, b = f64(o0_got).clone(), f64(o1_got).clone()
    a[-1] -= colsum_last
    b[0] += colsum_last
    return a, b


def mutate_count(loss_got):
    """mask count off by one"""
    m = f64(loss_got).clone()
    c = float(m[1])
    m[0] = m[0] * (c + 1e-8) / (c + 1 + 1e-8)
    m[1] = c + 1
    return m


def mutate_dpreds_offrow(dp_got, on: torch.Tensor):
    """dpreds non-zero on a row that is not a target (None when every row is one)"""
    off = torch.nonzero(on == 0)
    if off.numel() == 0:
        return None
    m = f64(dp_got).clone()
    m[int(off[0]), 0] = 2.0 ** -40
    return m


def mutate_drop_last_part(parts_got):
    """the last of the SPLIT group_stats parts dropped: returns the group totals [G][2]"""
    p = f64(parts_got).reshape(-1, SPLIT, 2).clone()
    p[:, SPLIT - 1] = 0
    return p.sum(1)


def ln_fwd_mutations(c, got, eps, kind):
    """[(label, output, mutated)] of the forward outputs `got` ({name: CPU tensor}) that apply to this input kind"""
    s = add_f32(c["x"], c["r"])
    M, D = s.shape
    out = []
    hows = {"randn": ("dm1",), "outlier": ("dm1",), "tiny": ("no_eps",), "offset": ("one_pass",)}.get(kind, ())
    coarse = c["x"].dtype == torch.bfloat16 and kind == "offset"
    if coarse:
        hows = ()           # bf16 rows at 1000 are small multiples of 4: their squares sum exactly in fp32, and narrow rows coincide
    for how in hows:
        y, rstd = mutate_ln_variance(got["y_f32"], got["rstd"], s, c["gamma"], c["beta"], eps, how)
        out += [(how + " y", "y_f32", y), (how + " rstd", "rstd", rstd)]
    last = (D - 1) // 4
    for row, chunk in ((0, 0), (M - 1, last)):
        out.append((f"chunk {chunk} of row {row} zero", "y_f32", mutate_chunk(got["y_f32"], row, chunk)))
    out.append(("chunk unwritten", "y_bf16", mutate_chunk(got["y_bf16"], M // 2, last, float("nan"))))
    if M > 1 and kind in ("randn", "offset", "outlier", "tiny") and not coarse:
        out.append(("rows swapped", "y_f32", mutate_swap_rows(got["y_f32"], M - 2)))
    if M > 1 and kind != "zero" and not coarse:
        out.append(("rows swapped (mean)", "mean", mutate_swap_rows(got["mean"], M - 2)))
    if D >= 36 or kind not in ("constant", "zero"):      # y = beta on such rows: four values may all truncate to what they round to
        out.append(("bf16 truncated", "y_bf16", mutate_truncate_bf16(got["y_f32"])))
    return out


def ln_bwd_mutations(got, terms, M):
    """column-sum and rounding mutations of the backward outputs; terms = (dy * xh, dy) fp64 rows of dgamma and dbeta"""
    dsb = f64(got["ds_bf16"])
    out = [("last row missing", "dgamma", mutate_colsum_row(got["dgamma"], terms[0][M - 1], -1)),
           ("last row missing", "dbeta", mutate_colsum_row(got["dbeta"], terms[1][M - 1], -1)),
           ("last row missing", "dbias", mutate_colsum_row(got["dbias"], dsb[M - 1], -1)),
           ("a row twice", "dbeta", mutate_colsum_row(got["dbeta"], terms[1][0], 1)),
           ("a row twice", "dbias", mutate_colsum_row(got["dbias"], dsb[0], 1)),
           ("dead second slot added", "dgamma", mutate_colsum_row(got["dgamma"], terms[0][M - 1], 1)),
           ("bf16 truncated", "ds_bf16", mutate_truncate_bf16(got["ds_f32"])),
           ("chunk zero", "ds_f32", mutate_chunk(got["ds_f32"], M - 1, (dsb.shape[1] - 1) // 4))]
    if M > 1:
        out.append(("rows swapped", "ds_f32", mutate_swap_rows(got["ds_f32"], 0)))
    return out


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
F = np.float32


def ln_shape(D: int) -> Tuple[int, int]:
    """(V, LPR) of ln_dispatch"""
    if D % 128 == 0 and D % 256 != 0 and D <= 384:
        return (1 if D == 128 else 3), 32
    return max(1, -(-D // 256)), 64


def _lanes(v: np.ndarray, D: int) -> np.ndarray:
    """[M][D] -> [M][LPR][V][4]: lane li holds columns li*4 + LPR*4*j .. +3 of chunk j (zeros outside the row)"""
    V, LPR = ln_shape(D)
    pad = np.zeros((v.shape[0], V * LPR * 4), dtype=F)
    pad[:, :D] = v
    return pad.reshape(v.shape[0], V, LPR, 4).transpose(0, 2, 1, 3)


def _butterfly(v: np.ndarray) -> np.ndarray:
    """[..., L] -> [...]: v += v[lane ^ o] for o = L/2 .. 1, as the shuffle reductions"""
    L = v.shape[-1]
    idx = np.arange(L)
    o = L // 2
    while o > 0:
        v = (v + v[..., idx ^ o]).astype(F)
        o >>= 1
    return v[..., 0]


def _lane_chain(t: np.ndarray, quads: bool) -> np.ndarray:
    """[M][LPR][V][4] -> [M][LPR]: a lane's own elements in order; quads: sum += ((a + b) + c) + d per chunk, else one by one"""
    acc = np.zeros(t.shape[:2], dtype=F)
    for j in range(t.shape[2]):
        if quads:
            q = ((t[:, :, j, 0] + t[:, :, j, 1]).astype(F) + t[:, :, j, 2]).astype(F)
            acc = (acc + (q + t[:, :, j, 3]).astype(F)).astype(F)
        else:
            for e in range(4):
                acc = (acc + t[:, :, j, e]).astype(F)
    return acc


def emu_row_sum(v: np.ndarray, D: int, quads: bool = False) -> np.ndarray:
    return _butterfly(_lane_chain(_lanes(v.astype(F), D), quads))


def _rsqrt(v: np.ndarray) -> np.ndarray:
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F)


def emulate_ln_fwd(x, r, gamma, beta, eps: float) -> Dict[str, np.ndarray]:
    s = add_f32(x, r).numpy().astype(F)
    D = s.shape[1]
    gamma, beta = gamma.numpy().astype(F), beta.numpy().astype(F)
    invD = F(1.0) / F(D)
    mean = (emu_row_sum(s, D, quads=True) * invD).astype(F)
    d = (s - mean[:, None]).astype(F)
    var = (emu_row_sum((d * d).astype(F), D) * invD).astype(F)
    rstd = _rsqrt((var + F(eps)).astype(F))
    y = ((((d * rstd[:, None]).astype(F)) * gamma).astype(F) + beta).astype(F)
    return {"s_f32": s, "y_f32": y, "y_bf16": torch.from_numpy(y).to(torch.bfloat16).float().numpy(), "mean": mean, "rstd": rstd}


def _chain_rows(t: np.ndarray) -> np.ndarray:
    """column sums as ONE fp32 chain over the rows (a worse order than any of the kernels')"""
    acc = np.zeros(t.shape[1], dtype=F)
    for m in range(t.shape[0]):
        acc = (acc + t[m]).astype(F)
    return acc


def emulate_ln_bwd(dy, s, gamma, mean, rstd, dres=None) -> Dict[str, np.ndarray]:
    """dy, s f32 [M][D] (already summed), mean / rstd the forward emulation's"""
    dy, s, gamma = dy.numpy().astype(F), s.numpy().astype(F), gamma.numpy().astype(F)
    D = s.shape[1]
    invD = F(1.0) / F(D)
    xh = ((s - mean[:, None]).astype(F) * rstd[:, None]).astype(F)
    g = (dy * gamma).astype(F)
    k1 = (emu_row_sum(g, D) * invD).astype(F)[:, None]
    k2 = (emu_row_sum((g * xh).astype(F), D) * invD).astype(F)[:, None]
    ds = (rstd[:, None] * ((g - k1).astype(F) - (xh * k2).astype(F)).astype(F)).astype(F)
    if dres is not None:
        ds = (dres.numpy().astype(F) + ds).astype(F)
    dsb = torch.from_numpy(ds).to(torch.bfloat16).float().numpy()
    return {"ds_f32": ds, "ds_bf16": dsb, "dgamma": _chain_rows((dy * xh).astype(F)), "dbeta": _chain_rows(dy), "dbias": _chain_rows(dsb)}


def emulate_colsum(x: torch.Tensor, out0: Optional[torch.Tensor] = None) -> np.ndarray:
    s = _chain_rows(x.float().numpy())
    return s if out0 is None else (out0.numpy().astype(F) + s).astype(F)


def emulate_group_stats(v: np.ndarray, group_rows: int, fma: bool, per_row: bool = True) -> np.ndarray:
    """[G][SPLIT][2] as store_group_stats leaves it: per lane a row's own elements, then the rows of its wave (per_row = False: ONE chain
    over all elements of all rows, the order that is 2.4 - 4.6 x over the bound on constant samples), the wave butterfly, the four waves"""
    M, D = v.shape
    V, LPR = ln_shape(D)
    rpw = 64 // LPR
    lanes = _lanes(v.astype(F), D).reshape(M, LPR, V * 4)
    G = -(-M // group_rows)
    rpp = -(-group_rows // SPLIT)
    out = np.zeros((G, SPLIT, 2), dtype=F)
    for g in range(G):
        for q in range(SPLIT):
            lo, hi = g * group_rows + q * rpp, min(M, g * group_rows + min(group_rows, (q + 1) * rpp))
            tot = np.zeros(2, dtype=F)
            for w in range(4):
                a1 = np.zeros((rpw, LPR), dtype=F)
                a2 = np.zeros((rpw, LPR), dtype=F)
                for sr in range(rpw):
                    for m in range(lo + w * rpw + sr, hi, 4 * rpw):
                        r1 = np.zeros(LPR, dtype=F) if per_row else a1[sr]
                        r2 = np.zeros(LPR, dtype=F) if per_row else a2[sr]
                        for e in range(V * 4):
                            t = lanes[m, :, e]
                            r1 = (r1 + t).astype(F)
                            sq = t.astype(np.float64) ** 2 + r2 if fma else (t * t).astype(F).astype(np.float64) + r2
                            r2 = sq.astype(F)
                        a1[sr] = (a1[sr] + r1).astype(F) if per_row else r1
                        a2[sr] = (a2[sr] + r2).astype(F) if per_row else r2
                w1 = _butterfly(a1.reshape(1, -1))[0]
                w2 = _butterfly(a2.reshape(1, -1))[0]
                tot = (tot + np.array([w1, w2], dtype=F)).astype(F)
            out[g, q] = tot
    return out


def _block_sum(x: np.ndarray) -> np.ndarray:
    """[B][n] -> [B]: 1024 threads, thread t takes float4 t, t + 1024, ...; wave butterflies, then the 16 waves in order"""
    Bn, n = x.shape
    it = -(-n // 4096)
    pad = np.zeros((Bn, it * 4096), dtype=F)
    pad[:, :n] = x
    pad = pad.reshape(Bn, it, 1024, 4)
    acc = np.zeros((Bn, 1024), dtype=F)
    for i in range(it):
        q = (((pad[:, i, :, 0] + pad[:, i, :, 1]).astype(F) + pad[:, i, :, 2]).astype(F) + pad[:, i, :, 3]).astype(F)
        acc = (acc + q).astype(F)
    waves = _butterfly(acc.reshape(Bn, 16, 64))
    tot = np.zeros(Bn, dtype=F)
    for w in range(16):
        tot = (tot + waves[:, w]).astype(F)
    return tot


def emulate_instnorm_accumulate(x, prev, scale: float, eps: float) -> np.ndarray:
    x = x.numpy().astype(F)
    n = F(x.shape[1])
    mean = (_block_sum(x) / n).astype(F)[:, None]
    d = (x - mean).astype(F)
    var = (_block_sum((d * d).astype(F)) / n).astype(F)[:, None]
    k = (_rsqrt((var + F(eps)).astype(F)) * F(scale)).astype(F)
    o = (d * k).astype(F)
    return o if prev is None else (o + prev.numpy().astype(F)).astype(F)


def emulate_instnorm_mean(xs, stats: np.ndarray, eps: float) -> np.ndarray:
    """stats [K][B][SPLIT][2] f32 (emulate_group_stats of each layer)"""
    K = len(xs)
    n = xs[0].shape[1]
    invn, invk = F(1.0) / F(n), F(1.0) / F(K)
    o = np.zeros(tuple(xs[0].shape), dtype=F)
    for l, x in enumerate(xs):
        s1 = np.zeros(stats.shape[1], dtype=F)
        s2 = np.zeros(stats.shape[1], dtype=F)
        for p in range(SPLIT):
            s1 = (s1 + stats[l, :, p, 0]).astype(F)
            s2 = (s2 + stats[l, :, p, 1]).astype(F)
        mu = (s1 * invn).astype(F)
        var = np.maximum(((s2 * invn).astype(F) - (mu * mu).astype(F)).astype(F), F(0))
        sc = (_rsqrt((var + F(eps)).astype(F)) * invk).astype(F)
        d = (x.numpy().astype(F) - mu[:, None]).astype(F)
        o = (d.astype(np.float64) * sc[:, None].astype(np.float64) + o).astype(F)     # fmaf
    return o


def emulate_masked_mse(preds, targets, tgt, B, G, T, D, gscale=1.0, gscale_dev=None, rows=None) -> Dict[str, np.ndarray]:
    p = preds.float().numpy().reshape(-1, D)
    y = targets.numpy().astype(F).reshape(B, T, D)
    on_dense = (tgt.reshape(-1) != 0).numpy()
    dense = np.arange(B * G * T) if rows is None else rows.numpy().astype(np.int64)
    p = p[:len(dense)]
    count = F(on_dense.sum())
    den = (count + F(1e-8)).astype(F)
    gk = F(2.0) / (F(D) * den).astype(F)
    gk = (gk * F(gscale)).astype(F)
    gk = (gk * (F(1.0) if gscale_dev is None else F(gscale_dev))).astype(F)
    on = on_dense[dense]
    b, t = (dense // T) // G, dense % T
    d = ((p - y[b, t]).astype(F) * on[:, None]).astype(F)
    sq = (d * d).astype(F)
    lanes = np.zeros((len(dense), 64), dtype=F)
    for c0 in range(0, D, 256):
        blk = np.zeros((len(dense), 256), dtype=F)
        w = min(256, D - c0)
        blk[:, :w] = sq[:, c0:c0 + w]
        blk = blk.reshape(len(dense), 64, 4)
        for e in range(4):
            lanes = (lanes + blk[:, :, e]).astype(F)
    err = (_butterfly(lanes) / F(D)).astype(F)
    # mse_final_kernel: thread t adds rows t, t + 1024, ... one by one, then block_sum
    acc = np.zeros(1024, dtype=F)
    for i in range(0, len(dense), 1024):
        seg = np.zeros(1024, dtype=F)
        seg[:len(err[i:i + 1024])] = err[i:i + 1024]
        acc = (acc + seg).astype(F)
    waves = _butterfly(acc.reshape(16, 64))
    tot = F(0)
    for w in range(16):
        tot = F(tot + waves[w])
    dp = torch.from_numpy((d * gk).astype(F)).to(torch.bfloat16).float().numpy()
    return {"loss": np.array([F(tot / den), count], dtype=F), "dpreds": dp}


# ------------------------------------------------------------------------------------------------------------ shared cases
def ln_inputs(kind: str, M: int, D: int, seed: int, with_r: bool, x_bf16: bool = False) -> dict:
    """x (f32 or bf16), r (bf16 or None), gamma, beta with s = x (+ r) of the given kind (the addend is a quarter of the row)"""
    base = make_rows(kind, M, D, seed)
    r = (base * 0.25).to(torch.bfloat16) if with_r else None
    x = base - r.float() if with_r else base
    if x_bf16:
        x = x.to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 1000)
    return dict(x=x, r=r, gamma=1 + 0.1 * torch.randn(D, generator=g), beta=0.1 * torch.randn(D, generator=g),
                dy=torch.randn(M, D, generator=g), dy2=torch.randn(M, D, generator=g), dres=torch.randn(M, D, generator=g))


def colsum_input(kind: str, M: int, N: int, seed: int) -> torch.Tensor:
    """randn, or a cancelling column: +-1e4 alternating down the rows plus randn"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, N, generator=g)
    if kind == "cancel":
        x = x + 1e4 * (1 - 2 * (torch.arange(M) % 2).float())[:, None]
    return x


RATIOS = (0.0, 3.0, 30.0)      # mean / sigma of the teacher layers


def instnorm_layers(B: int, TD: int, K: int, seed: int) -> List[torch.Tensor]:
    """K layers [B][TD]: layer l has mean / sigma = RATIOS[l % 3] at sigma = 1 + l / 2; the last sample of layer 0 is constant"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for l in range(K):
        sig = 1.0 + 0.5 * l
        x = (torch.randn(B, TD, generator=g) + RATIOS[l % 3]) * sig
        if l == 0:
            x[B - 1] = 0.7371
        out.append(x)
    return out


MASK_BYTES = (0, 1, 2, 255)


def mse_inputs(B: int, G: int, T: int, D: int, seed: int, mask: str = "mixed") -> dict:
    g = torch.Generator().manual_seed(seed)
    preds = torch.randn(B * G * T, D, generator=g).to(torch.bfloat16)
    targets = torch.randn(B, T, D, generator=g)
    n = B * G * T
    if mask == "mixed":
        tgt = torch.tensor(MASK_BYTES, dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=g)]
    else:
        tgt = torch.full((n,), 0 if mask == "zeros" else 1, dtype=torch.uint8)
    return dict(preds=preds, targets=targets, tgt=tgt)
