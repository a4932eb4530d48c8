"""fp64 reference, per-element error bounds, fp32 emulation and mutations for conv layer 0 in the default mode: wj_conv0_gn_gelu_fwd /
wj_conv0_gn_gelu_bwd (csrc/conv0.hip).  Test infrastructure; used by tests/test_conv0_reference_cpu.py and tests/test_conv0_bounds_gpu.py.

Every reference function takes the operands of one call as CPU tensors and returns {output: (fp64 reference, bound)}; `check` of
tests/norm_reference.py requires every element finite and within its bound.  There is no norm anywhere.

Rounding points (read off csrc/conv0.hip), x_{t,q} = audio[ci][t stride + kk], q = ci k + kk:
  yu_t  = sum_q w_q x_{t,q}                  exact in fp64 (products of bf16 values); the kernels accumulate it in fp32
  y_t   = bf16(yu_t)                         the conv output is a bf16 tensor; every pass that needs it recomputes it from the audio
  statistics over t < L_out, biased:         mu = fl32(s1 / L), var = max(fl32(s2 / L - mu^2), 0), rstd = rsqrt(var + eps), with
      "gram"      s1 = sum yu, s2 = sum yu^2, yx_q = sum yu x_q, x1_q = sum x_q   from the clip's patch Gram matrix in fp64: the UNROUNDED yu
      "fallback"  the same sums of the ROUNDED y, accumulated in fp32 (conv0_stats_mfma_kernel)
  z     = (y - mu) rstd gamma + beta         (MFMA apply: y ka + kb with ka = fl32(rstd gamma), kb = fl32(beta - mu ka))
  act_t = bf16(gelu(z_t)) for t < L_out, exactly 0 for L_out <= t < P
The backward is DEFINED on the stored mean / rstd / yx / x1 of the forward launch (as the LayerNorm backward bound is on its stored
statistics): with xh = (y - mean) rstd, z = xh gamma + beta, dz = dact gelu'(z) on the listed rows (every row t < L_out in the dense form),
  A1 = sum_t dz, A2 = sum_t dz xh, S_q = sum_t dz x_q
  dbeta += sum_n A1, dgamma += sum_n A2, dw_q += sum_n rstd gamma [S_q - (A1 / L) x1_q - (A2 / L) rstd (yx_q - mean x1_q)]
which is autograd of conv1d -> group_norm -> gelu with the bf16 rounding of y straight-through when the statistics are those of y.

Bounds: first-order propagation, term by term, u = 2^-24, KAPPA of tests/norm_reference.py.
  y     : yu is known to the kernels within dy0 = KAPPA u sum_q |w_q x_q|; where [yu - dy0, yu + dy0] holds a bf16 rounding boundary the
          kernel's y may be the neighbouring bf16 value: dy = max |bf16(yu +- dy0) - y| (zero elsewhere, as in bf16_bound)
  mean  : dmu = KAPPA u mean|y| + mean dy + 3 u |mu|  (+ 2^-50 mean sum_q|w_q x_q| for the fp64 Gram)
  var   : one pass, so it carries kappa = (s2 / L) / (var + eps) (as instnorm_mean): dvar = 2 KAPPA u kappa (var + eps) + mean(2 |y| dy)
          + 2 |mu| mean dy (+ 2^-50 mean (sum_q|w_q x_q|)^2);   drstd / rstd = KAPPA u + dvar / (2 (var + eps))
  z     : dc = u |c| + dmu + dy;  dxh = rstd dc + |xh| drstd / rstd;  dz = |gamma| dxh + 3 u (|gamma xh| + |beta|), and the folded affine of
          the MFMA apply adds u (|y| + |mu|) rstd |gamma|
  act   : GELU as the CONV_GELU branch of tests/gemm_reference.py: eg = min(|gelu'(z)| + GELU2 dz, GELU1) dz + ERF_APPROX |z| + u |g|, then
          bf16_bound(g, eg); padding rows: bound 0
  yx, x1: 2 u |.| for the fp64 Gram (one fp32 rounding attains u; + its 2^-50 term); KAPPA u sum|term| + sum_t dy |x_q| for the fallback
  backward terms: dxh = rstd (u |c| + dy) + 2 u |xh| (stored statistics: no dmu); dz_ = |gamma| dxh + 3 u (|gamma xh| + |beta|);
          gelu' carries min(|gelu''(z)| + GELU3 dz_, GELU2) dz_ + ERF_APPROX (1 + |z|) + u |gelu'|;  T = dact gelu'(z): dT = |dact| dgelu' + u |T|
  A1, A2, S_q: KAPPA u sum_t |term| + the propagated dT (A2 also sum |T| dxh)
  dw    : over t1 = rstd gamma S, t2 = rstd gamma A1 x1 / L, t3 = rstd^2 gamma A2 (yx - mean x1) / L SEPARATELY -- t3 carries
          u (|yx| + 2 |mean x1|), which exceeds |yx - mean x1| when a channel has a large mean: the cancellation is visible in the bound
  the accumulators: u |initial| + u |result| + KAPPA u sum_n |term|
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.gemm_reference import ERF_APPROX, GELU1, GELU2, GELU3, gelu, gelu1, gelu2
from tests.norm_reference import KAPPA, U, Guarded, bf16, bf16_bound, check, f32eps, f64, guarded_like, rejected, worst  # noqa: F401

Pair = Tuple[torch.Tensor, torch.Tensor]
F = np.float32
U64 = 2.0 ** -50          # a few fp64 roundings of the Gram sums

HANDLED = {
    "wj_conv0_fwd_args": {"audio", "w", "gamma", "beta", "act", "mean", "rstd", "workspace", "yx", "x1", "audio_clip_stride", "N", "C_in", "L",
                          "C", "k", "stride", "L_out", "P", "eps"},
    "wj_conv0_bwd_args": {"audio", "w", "gamma", "beta", "mean", "rstd", "dact", "yx", "x1", "rows", "row_off", "dw", "dgamma", "dbeta",
                          "workspace", "audio_clip_stride", "N", "C_in", "L", "C", "k", "stride", "L_out", "P", "max_rows"},
}
EXCLUDED: Dict[str, Dict[str, str]] = {}

KINDS = ("randn", "offset", "tiny", "zero", "constant", "highpass", "gamma0", "tails")
STATS_SLOTS = 768
TC, TCA, BR = 256, 512, 256


# ------------------------------------------------------------------------------------------------------------ geometry
def stats_tcs(N: int, L_out: int, C_in: int) -> int:
    """time steps per workgroup of the forward statistics pass (stats_tcs of csrc/conv0.hip)"""
    chunks = (STATS_SLOTS + N // 2) // N
    most = (L_out + 255) // 256
    chunks = max(1, min(chunks, most))
    tcs = ((L_out + chunks - 1) // chunks + 31) // 32 * 32
    cap = 2176 // C_in // 32 * 32
    return max(cap, 32) if tcs > cap else tcs


def stats_form(N: int, C_in: int, C: int, L_out: int, k: int = 10) -> dict:
    """the statistics form launch_fwd takes: {"form": "gram" | "fallback", "tcs", "chunks", "rec", "ws_bytes"}"""
    taps = C_in * k
    tcs = stats_tcs(N, L_out, C_in)
    chunks = (L_out + tcs - 1) // tcs
    rec = 2 * C + C * taps + taps
    G = taps + taps * taps
    gram = 2 * G * (chunks + 1) <= chunks * rec
    return {"form": "gram" if gram else "fallback", "tcs": tcs, "chunks": chunks, "rec": rec, "ws_bytes": (2 * N * C + N * chunks * rec) * 4}


def apply_form(C: int) -> str:
    return "mfma" if C % 64 == 0 else "valu"


def patches(audio: torch.Tensor, k: int, stride: int, L_out: int) -> torch.Tensor:
    """audio [N][C_in][L] -> fp64 [N][L_out][C_in k]"""
    a = f64(audio)
    N = a.shape[0]
    return a[:, :, :(L_out - 1) * stride + k].unfold(2, k, stride).permute(0, 2, 1, 3).reshape(N, L_out, -1)


def _conv(audio, w, geo, y=None):
    """patches, weights, the exact conv output, sum_q |w_q x_q|, y = bf16(yu) and its straddle interval dy.  y given (the y of an
    emulation, [N][L_out][C]): it is taken as it is, dy = 0 -- the margin of the accumulation terms alone (tests/test_conv0_reference_cpu.py)"""
    X = patches(audio, geo["k"], geo["stride"], geo["L_out"])            # [N][Lo][T]
    W = f64(w).reshape(w.shape[0], -1)                                      # [C][T]
    yu = X @ W.t()                                                          # [N][Lo][C]
    sab = X.abs() @ W.abs().t()
    dy0 = KAPPA * U * sab
    if y is not None:
        return X, W, yu, sab, f64(y), torch.zeros_like(yu)
    y = bf16(yu)
    dy = torch.maximum((bf16(yu + dy0) - y).abs(), (bf16(yu - dy0) - y).abs())
    return X, W, yu, sab, y, dy


# ------------------------------------------------------------------------------------------------------------ forward
def conv0_fwd(audio, w, gamma, beta, eps: float, geometry: dict, stats_form, y=None) -> Dict[str, Pair]:
    """wj_conv0_gn_gelu_fwd.  audio bf16 [N][C_in][L] (the clips as the call sees them: one channel of a strided batch is [N][1][L]),
    w bf16 [C][C_in][k], gamma / beta f32 [C]; geometry = {k, stride, L_out, P}; stats_form "gram" / "fallback" (or stats_form()'s dict).
    Returns act [N][P][C], mean / rstd [N][C], yx [N][C][taps], x1 [N][taps], and "kappa" [N][C] (bound slot: zeros)."""
    form = stats_form["form"] if isinstance(stats_form, dict) else stats_form
    assert form in ("gram", "fallback")
    eps = f32eps(eps)
    L_out, P = geometry["L_out"], geometry["P"]
    gamma, beta = f64(gamma), f64(beta)
    X, W, yu, sab, y, dy = _conv(audio, w, geometry, y)
    N, _, C = y.shape
    v = yu if form == "gram" else y                       # what the statistics are the statistics of
    dv = torch.zeros_like(dy) if form == "gram" else dy
    mu = v.mean(1)
    var = ((v - mu[:, None]) ** 2).mean(1)
    s2n = (v * v).mean(1)
    kappa = s2n / (var + eps)
    rstd = 1.0 / torch.sqrt(var + eps)
    e64 = U64 if form == "gram" else 0.0
    dmu = KAPPA * U * v.abs().mean(1) + dv.mean(1) + 3 * U * mu.abs() + e64 * sab.mean(1)
    dvar = 2 * KAPPA * U * kappa * (var + eps) + (2 * v.abs() * dv).mean(1) + 2 * mu.abs() * dv.mean(1) + e64 * (sab * sab).mean(1)
    drel = KAPPA * U + dvar / (2 * (var + eps))
    c = y - mu[:, None]
    xh = c * rstd[:, None]
    dc = U * c.abs() + dmu[:, None] + dy
    dxh = rstd[:, None] * dc + xh.abs() * drel[:, None]
    z = xh * gamma + beta
    dz = gamma.abs() * dxh + 3 * U * ((gamma * xh).abs() + beta.abs()) + U * (y.abs() + mu[:, None].abs()) * rstd[:, None] * gamma.abs()
    g = gelu(z)
    eg = torch.clamp(gelu1(z).abs() + GELU2 * dz, max=GELU1) * dz + ERF_APPROX * z.abs() + U * g.abs()
    act = torch.zeros(N, P, C, dtype=torch.float64)
    bact = torch.zeros(N, P, C, dtype=torch.float64)
    act[:, :L_out] = bf16(g)
    bact[:, :L_out] = bf16_bound(g, eg)
    yx = torch.einsum("ntc,ntq->ncq", v, X)
    x1 = X.sum(1)
    if form == "gram":
        byx = 2 * U * yx.abs() + U64 * torch.einsum("ntc,ntq->ncq", sab, X.abs())      # ONE fp32 rounding attains u: an ulp's worth
        bx1 = 2 * U * x1.abs() + U64 * X.abs().sum(1)
    else:
        byx = KAPPA * U * torch.einsum("ntc,ntq->ncq", v.abs(), X.abs()) + torch.einsum("ntc,ntq->ncq", dy, X.abs())
        bx1 = KAPPA * U * X.abs().sum(1)
    return {"act": (act, bact), "mean": (mu, dmu), "rstd": (rstd, rstd * (drel + U)), "yx": (yx, byx), "x1": (x1, bx1),
            "kappa": (kappa, torch.zeros_like(kappa)), "_y": (y, dy), "_form": form}


# ------------------------------------------------------------------------------------------------------------ backward
def live_mask(N: int, L_out: int, lists: Optional[List[List[int]]]) -> torch.Tensor:
    """[N][L_out] bool: the listed rows of every clip (None: the dense form, every row)"""
    if lists is None:
        return torch.ones(N, L_out, dtype=torch.bool)
    m = torch.zeros(N, L_out, dtype=torch.bool)
    for n, tl in enumerate(lists):
        m[n, torch.tensor(tl, dtype=torch.long)] = True
    return m


def row_lists(lists: List[List[int]], P: int) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """rows (global indices n P + t, ascending), row_off [N + 1], the longest list"""
    rows = [n * P + t for n, tl in enumerate(lists) for t in tl]
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(tl) for tl in lists])
    return torch.tensor(rows, dtype=torch.int32), torch.from_numpy(off).to(torch.int32), max([len(tl) for tl in lists] + [0])


def _bwd_sums(ctx: dict, how: str = "") -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(dw [C][T], dgamma, dbeta) WITHOUT the accumulators' initial contents; `how` selects one of the wrong formulas of the mutations"""
    X, y, d, live = ctx["X"], ctx["y"], ctx["d"], ctx["live"]
    mu, rs, ga, be, yx, x1 = ctx["mean"], ctx["rstd"], ctx["gamma"], ctx["beta"], ctx["yx"], ctx["x1"]
    L_out = y.shape[1]
    if how == "rows256":                      # rows 256.. of every clip's list dropped
        live = live & (live.long().cumsum(1) <= BR)
    if how == "unlisted":                     # the first unlisted row included, with a gradient of 1
        n, t = [int(v) for v in torch.nonzero(~live)[0]]
        live = live.clone()
        live[n, t] = True
        d = d.clone()
        d[n, t] = 1.0
    m = live.double()[:, :, None]
    xh = (y - mu[:, None]) * rs[:, None]
    z = xh * ga + be
    T = torch.nan_to_num(d) * gelu1(xh if how == "gelu_at_xh" else z) * m
    A1, A2 = T.sum(1), (T * xh).sum(1)                      # [N][C]
    S = torch.einsum("ntc,ntq->ncq", T, X)
    invL = 1.0 / (ctx["P"] if how == "invP" else L_out)
    scale = torch.ones_like(rs) if how == "no_scale" else rs * ga
    t3 = 0.0 if how == "no_a2" else (A2 * invL * rs)[:, :, None] * (yx - mu[:, :, None] * x1[:, None, :])
    per = scale[:, :, None] * (S - (A1 * invL)[:, :, None] * x1[:, None, :] - t3)
    nmax = 8 if how == "clips8" else y.shape[0]
    return per[:nmax].sum(0), A2[:nmax].sum(0), A1[:nmax].sum(0)


def conv0_bwd(audio, w, gamma, beta, mean, rstd, yx, x1, dact, geometry: dict, lists: Optional[List[List[int]]] = None,
              dw0=None, dgamma0=None, dbeta0=None, y=None, reuse: Optional[dict] = None) -> Dict[str, Pair]:
    """wj_conv0_gn_gelu_bwd on the STORED mean / rstd / yx / x1 of the forward launch.  dact bf16 [N][P][C]: read on the listed rows only
    (lists: per clip the ascending time steps; None: the dense form); dw0 / dgamma0 / dbeta0: what the accumulators held before.
    reuse: the result of an earlier call on the same operands (other initial contents): the sums and their bounds are taken from it."""
    if reuse is not None:
        return _with_initial(reuse["_core"], dw0, dgamma0, dbeta0)
    L_out, P = geometry["L_out"], geometry["P"]
    gamma, beta = f64(gamma), f64(beta)
    X, W, yu, sab, y, dy = _conv(audio, w, geometry, y)
    N, _, C = y.shape
    Tn = X.shape[2]
    mean, rstd, yx, x1 = f64(mean).reshape(N, C), f64(rstd).reshape(N, C), f64(yx).reshape(N, C, Tn), f64(x1).reshape(N, Tn)
    live = live_mask(N, L_out, lists)
    d = f64(dact).reshape(N, P, C)[:, :L_out]
    ctx = dict(X=X, y=y, d=d, live=live, mean=mean, rstd=rstd, gamma=gamma, beta=beta, yx=yx, x1=x1, P=P)
    dw, dg, db = _bwd_sums(ctx)
    # bounds
    m = live.double()[:, :, None]
    d = torch.nan_to_num(d) * m
    rs, mu = rstd[:, None], mean[:, None]
    c = y - mu
    xh = c * rs
    dxh = rs * (U * c.abs() + dy) + 2 * U * xh.abs()
    z = xh * gamma + beta
    dz = gamma.abs() * dxh + 3 * U * ((gamma * xh).abs() + beta.abs())
    gp = gelu1(z)
    dgp = torch.clamp(gelu2(z).abs() + GELU3 * dz, max=GELU2) * dz + ERF_APPROX * (1 + z.abs()) + U * gp.abs()
    T = d * gp
    dT = d.abs() * dgp + U * T.abs()
    bA1 = KAPPA * U * T.abs().sum(1) + dT.sum(1)
    bA2 = (KAPPA + 1) * U * (T * xh).abs().sum(1) + (dT * xh.abs() + T.abs() * dxh).sum(1)
    bS = (KAPPA + 1) * U * torch.einsum("ntc,ntq->ncq", T.abs(), X.abs()) + torch.einsum("ntc,ntq->ncq", dT, X.abs())
    A1, A2 = T.sum(1), (T * xh).sum(1)
    S = torch.einsum("ntc,ntq->ncq", T, X)
    invL = 1.0 / L_out
    sc = (rstd * gamma).abs()[:, :, None]
    X1 = x1[:, None, :]
    D = yx - mean[:, :, None] * X1
    bD = U * (yx.abs() + 2 * (mean[:, :, None] * X1).abs())
    t1 = sc * S.abs()
    t2 = sc * (A1[:, :, None] * X1).abs() * invL
    t3 = sc * (rstd * A2).abs()[:, :, None] * D.abs() * invL
    b1 = sc * bS
    b2 = sc * bA1[:, :, None] * X1.abs() * invL
    b3 = sc * rstd[:, :, None] * invL * (bA2[:, :, None] * D.abs() + A2.abs()[:, :, None] * bD)
    per = b1 + b2 + b3 + 6 * U * (t1 + t2 + t3)
    mag = t1 + t2 + t3
    parts = {"t1": t1.sum(0), "t2": t2.sum(0), "t3": t3.sum(0), "b1": b1.sum(0), "b2": b2.sum(0), "b3": b3.sum(0)}
    core = dict(ctx=ctx, parts=parts, dw=(dw, per.sum(0), mag.sum(0)), dgamma=(dg, bA2.sum(0), A2.abs().sum(0)),
                dbeta=(db, bA1.sum(0), A1.abs().sum(0)))
    return _with_initial(core, dw0, dgamma0, dbeta0)


def _with_initial(core: dict, dw0, dgamma0, dbeta0) -> Dict[str, Pair]:
    out = {}
    ctx = dict(core["ctx"])
    for name, key, init in (("dw", "dw0", dw0), ("dgamma", "dg0", dgamma0), ("dbeta", "db0", dbeta0)):
        ref, b, mg = core[name]
        init = torch.zeros_like(ref) if init is None else f64(init).reshape(ref.shape)
        ctx[key] = init
        r = init + ref
        out[name] = (r, b + KAPPA * U * mg + U * init.abs() + U * r.abs())
    out["_ctx"] = ctx
    out["_parts"] = core["parts"]
    out["_core"] = core
    return out


# ------------------------------------------------------------------------------------------------------------ mutations
def fwd_mutations(ref: Dict[str, Pair], got: Dict[str, torch.Tensor], gamma, beta, eps: float, geometry: dict, kind: str,
                  distinct_clips: bool = True) -> List[Tuple[str, str, torch.Tensor]]:
    """[(label, output, mutated fp64 copy)] of a correct forward output `got` ({name: CPU tensor}), the ones that apply to this case"""
    L_out, P = geometry["L_out"], geometry["P"]
    eps = f32eps(eps)
    y = ref["_y"][0]
    N, _, C = y.shape
    gamma, beta = f64(gamma), f64(beta)
    mu, rstd = ref["mean"][0], ref["rstd"][0]
    var = 1.0 / (rstd * rstd) - eps
    act, mean_g, rstd_g = f64(got["act"]).reshape(N, P, C), f64(got["mean"]).reshape(N, C), f64(got["rstd"]).reshape(N, C)
    out = []

    def act_with(mu_, rstd_):
        a = act.clone()
        right = bf16(gelu((y - mu[:, None]) * rstd[:, None] * gamma + beta))
        wrong = bf16(gelu((y - mu_[:, None]) * rstd_[:, None] * gamma + beta))
        a[:, :L_out] += wrong - right
        return a

    live_kind = kind not in ("zero", "constant")
    if L_out > 1 and live_kind:
        r1 = 1.0 / torch.sqrt(var * L_out / (L_out - 1) + eps)
        out.append(("unbiased variance", "rstd", rstd_g + (r1 - rstd)))
        if L_out <= 17:
            out.append(("unbiased variance", "act", act_with(mu, r1)))
    if kind == "tiny":
        r1 = 1.0 / torch.sqrt(var.clamp_min(1e-300))
        out.append(("eps left out", "rstd", rstd_g + (r1 - rstd)))
        if L_out > 1:                     # one time step: y = mu, the activation does not depend on rstd
            out.append(("eps left out", "act", act_with(mu, r1)))
    if L_out > 1 and live_kind:
        out.append(("last time step missing from the statistics", "mean", mean_g - y[:, L_out - 1] / L_out))
    if N > 1 and distinct_clips and live_kind:
        out.append(("statistics of clip n + 1", "mean", torch.roll(mean_g, -1, 0)))
        if L_out > 1:                     # one time step: var = 0 and rstd = rsqrt(eps) in every clip
            out.append(("statistics of clip n + 1", "rstd", torch.roll(rstd_g, -1, 0)))
        out.append(("statistics of clip n + 1", "act", act_with(torch.roll(mu, -1, 0), torch.roll(rstd, -1, 0))))
    if C >= 8:
        for t, c4 in ((0, 0), (L_out - 1, C - 8)):
            a = act.clone()
            a[N - 1, t, c4:c4 + 4], a[N - 1, t, c4 + 4:c4 + 8] = act[N - 1, t, c4 + 4:c4 + 8], act[N - 1, t, c4:c4 + 4]
            out.append((f"4-channel group {c4 // 4} swapped with its neighbour on row {t}", "act", a))
    a = act.clone()
    a[:, L_out - 1] = 0
    out.append(("row L_out - 1 zeroed", "act", a))
    if P > L_out:
        for t in (L_out, P - 1):
            a = act.clone()
            a[N - 1, t, C - 1] = 2.0 ** -40
            out.append((f"padding row {t} non-zero", "act", a))
    for tile in (TC, TCA):
        if L_out > tile and live_kind:
            a = act.clone()
            a[:, tile] = act[:, tile - 1]
            out.append((f"first row of the second {tile} tile taken from the tile before", "act", a))
    return out


def bwd_mutations(ref: Dict[str, Pair], got: Dict[str, torch.Tensor], kind: str = "randn") -> List[Tuple[str, str, torch.Tensor]]:
    """[(label, output, mutated fp64 copy)] of a correct backward output `got` = {dw, dgamma, dbeta}.  kind "constant": every patch of a
    clip is the same and xh = 0, so dgamma = 0 and dw = rstd gamma (S - A1 x1 / L) = 0 under every formula below: dbeta alone is mutated."""
    ctx = ref["_ctx"]
    N, L_out = ctx["y"].shape[:2]
    right = dict(zip(("dw", "dgamma", "dbeta"), _bwd_sums(ctx)))
    g = {k: f64(got[k]).reshape(right[k].shape) for k in right}
    out = []

    def add(label, how, names):
        wrong = dict(zip(("dw", "dgamma", "dbeta"), _bwd_sums(ctx, how)))
        for k in names:
            if (L_out == 1 or kind == "constant") and k != "dbeta":   # one time step: xh = 0 as well
                continue
            out.append((label, k, g[k] + (wrong[k] - right[k])))

    live_rows = int(ctx["live"].sum())
    if live_rows:
        add("gelu' evaluated at xh instead of z", "gelu_at_xh", ("dw", "dgamma", "dbeta"))
        add("the A2 term dropped", "no_a2", ("dw",))
        add("the factor rstd gamma missing", "no_scale", ("dw",))
        if ctx["P"] != L_out:
            add("1 / P for 1 / L_out", "invP", ("dw",))
        if N > 8 and int(ctx["live"][8:].sum()):
            add("clips 8.. dropped", "clips8", ("dw", "dgamma", "dbeta"))
        if int(ctx["live"].sum(1).max()) > BR:
            add("rows 256.. of a clip dropped", "rows256", ("dw", "dgamma", "dbeta"))
    if not bool(ctx["live"].all()):
        add("one unlisted row included", "unlisted", ("dw", "dgamma", "dbeta"))
    for k, init in (("dw", ctx["dw0"]), ("dgamma", ctx["dg0"]), ("dbeta", ctx["db0"])):
        if bool((init != 0).any()):
            out.append(("= for +=", k, g[k] - init))
    return out


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def _np(t) -> np.ndarray:
    return t.detach().cpu().float().numpy().astype(F)


def _fma(a, b, c) -> np.ndarray:
    """fl32(a b + c) for f32 operands (the product is exact in fp64)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _bf16_np(a: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to(torch.bfloat16).float().numpy()


def _rsqrt(v: np.ndarray) -> np.ndarray:
    return (1.0 / np.sqrt(v.astype(np.float64))).astype(F)


def _conv_f32(X: np.ndarray, W: np.ndarray) -> np.ndarray:
    """[..][T] x [C][T] -> bf16-rounded [..][C]: one fp32 fma chain over the taps"""
    a = np.zeros(X.shape[:-1] + (W.shape[0],), dtype=F)
    for tp in range(W.shape[1]):
        a = _fma(X[..., tp, None], W[:, tp], a)
    return _bf16_np(a)


def _lanes4(v: np.ndarray) -> np.ndarray:
    """per-lane partials [4][...] -> (g0 + g1) + (g2 + g3): the xor-16 / xor-32 butterfly as lane 0 sees it"""
    return ((v[0] + v[1]).astype(F) + (v[2] + v[3]).astype(F)).astype(F)


def emulate_fwd(audio, w, gamma, beta, eps: float, geometry: dict, form: dict) -> Dict[str, np.ndarray]:
    """fp32 numpy in the kernels' order: the statistics per chunk of form["tcs"] steps, folded in chunk order (fp64 sums in the Gram form;
    in the fallback a lane's own steps, then the butterfly over the four lane groups), then the VALU or the folded MFMA apply by C % 64."""
    k, stride, L_out, P = geometry["k"], geometry["stride"], geometry["L_out"], geometry["P"]
    X64 = patches(audio, k, stride, L_out).numpy()
    X = X64.astype(F)
    W = _np(w).reshape(w.shape[0], -1)
    N, _, Tn = X.shape
    C = W.shape[0]
    ga, be = _np(gamma), _np(beta)
    y = _conv_f32(X, W)                                     # [N][Lo][C]
    tcs = form["tcs"]
    if form["form"] == "gram":
        W64 = W.astype(np.float64)
        g1 = np.zeros((N, Tn))
        g2 = np.zeros((N, Tn, Tn))
        for t0 in range(0, L_out, tcs):
            xc = X64[:, t0:t0 + tcs]
            g1 = g1 + xc.sum(1)
            g2 = g2 + np.einsum("ntk,ntq->nkq", xc, xc)
        s1 = (g1 @ W64.T).astype(F)
        v = np.einsum("ck,nkq->ncq", W64, g2)
        s2 = np.maximum((v * W64[None]).sum(2), 0.0).astype(F)
        yx, x1 = v.astype(F), g1.astype(F)
    else:
        s1 = np.zeros((N, C), dtype=F)
        s2 = np.zeros((N, C), dtype=F)
        yx = np.zeros((N, C, Tn), dtype=F)
        x1 = np.zeros((N, Tn), dtype=F)
        for t0 in range(0, L_out, tcs):
            tc = min(tcs, L_out - t0)
            nb = -(-tc // 32)
            yp = np.zeros((N, nb * 32, C), dtype=F)
            xp = np.zeros((N, nb * 32, Tn), dtype=F)
            yp[:, :tc], xp[:, :tc] = y[:, t0:t0 + tc], X[:, t0:t0 + tc]
            yb = yp.reshape(N, nb, 2, 4, 4, C)              # block, d0 / d1, lane group, r
            xb = xp.reshape(N, nb, 2, 4, 4, Tn)
            a1 = np.zeros((4, N, C), dtype=F)
            a2 = np.zeros((4, N, C), dtype=F)
            ax = np.zeros((4, N, Tn), dtype=F)
            ayx = np.zeros((N, C, Tn), dtype=F)
            for b in range(nb):
                for r in range(4):
                    a, bb = np.moveaxis(yb[:, b, 0, :, r], 1, 0), np.moveaxis(yb[:, b, 1, :, r], 1, 0)    # [4][N][C]
                    a1 = (a1 + (a + bb).astype(F)).astype(F)
                    a2 = _fma(a, a, _fma(bb, bb, a2))
                for h in range(2):
                    for r in range(4):
                        ax = (ax + np.moveaxis(xb[:, b, h, :, r], 1, 0)).astype(F)
                blk = slice(b * 32, b * 32 + 32)
                ayx = (ayx + np.einsum("ntc,ntq->ncq", yp[:, blk].astype(np.float64), xp[:, blk].astype(np.float64))).astype(F)
            s1 = (s1 + _lanes4(a1)).astype(F)
            s2 = (s2 + _lanes4(a2)).astype(F)
            x1 = (x1 + _lanes4(ax)).astype(F)
            yx = (yx + ayx).astype(F)
    invL = F(1.0) / F(L_out)
    mu = (s1 * invL).astype(F)
    var = np.maximum(((s2 * invL).astype(F) - (mu * mu).astype(F)).astype(F), F(0))
    rs = _rsqrt((var + F(eps)).astype(F))
    if apply_form(C) == "mfma":
        ka = (rs * ga).astype(F)
        kb = _fma(-mu, ka, be)
        z = _fma(y, ka[:, None], kb[:, None])
    else:
        z = ((((y - mu[:, None]).astype(F) * rs[:, None]).astype(F) * ga).astype(F) + be).astype(F)
    g = gelu(torch.from_numpy(z.astype(np.float64))).numpy().astype(F)
    act = np.zeros((N, P, C), dtype=F)
    act[:, :L_out] = _bf16_np(g)
    return {"act": act, "mean": mu, "rstd": rs, "yx": yx, "x1": x1, "_y": y}


def emulate_bwd(audio, w, gamma, beta, mean, rstd, yx, x1, dact, geometry: dict, lists: Optional[List[List[int]]] = None,
                dw0=None, dgamma0=None, dbeta0=None) -> Dict[str, np.ndarray]:
    """fp32 numpy in the kernels' order: a clip's listed rows in chunks of 256, the even and the odd rows of a chunk as two chains added
    last, the chunks folded in chunk order, then eight clip lanes (n, n + 8, ...) and their fold, added into the accumulators."""
    k, stride, L_out, P = geometry["k"], geometry["stride"], geometry["L_out"], geometry["P"]
    X = patches(audio, k, stride, L_out).numpy().astype(F)
    W = _np(w).reshape(w.shape[0], -1)
    N, _, Tn = X.shape
    C = W.shape[0]
    ga, be = _np(gamma), _np(beta)
    mean, rstd, yx, x1 = _np(mean).reshape(N, C), _np(rstd).reshape(N, C), _np(yx).reshape(N, C, Tn), _np(x1).reshape(N, Tn)
    d_all = torch.nan_to_num(dact.detach().cpu().float()).numpy().astype(F).reshape(N, P, C)
    A1 = np.zeros((N, C), dtype=F)
    A2 = np.zeros((N, C), dtype=F)
    S = np.zeros((N, C, Tn), dtype=F)
    y_all = _conv_f32(X, W)
    for n in range(N):
        tl = np.arange(L_out) if lists is None else np.asarray(lists[n], dtype=np.int64)
        cnt = len(tl)
        if cnt == 0:
            continue
        nch = -(-cnt // BR)
        x = np.zeros((nch * BR, Tn), dtype=F)
        x[:cnt] = X[n, tl]
        d = np.zeros((nch * BR, C), dtype=F)
        d[:cnt] = d_all[n, tl]
        y = np.zeros((nch * BR, C), dtype=F)
        y[:cnt] = y_all[n, tl]
        xh = ((y - mean[n]).astype(F) * rstd[n]).astype(F)
        z = ((xh * ga).astype(F) + be).astype(F)
        gp = gelu1(torch.from_numpy(z.astype(np.float64))).numpy().astype(F)
        dz = (d * gp).astype(F)
        dz, xh, x = dz.reshape(nch, BR // 2, 2, C), xh.reshape(nch, BR // 2, 2, C), x.reshape(nch, BR // 2, 2, Tn)
        a1 = np.zeros((nch, 2, C), dtype=F)
        a2 = np.zeros((nch, 2, C), dtype=F)
        acc = np.zeros((nch, 2, C, Tn), dtype=F)
        for i in range(BR // 2):
            a1 = (a1 + dz[:, i]).astype(F)
            a2 = _fma(dz[:, i], xh[:, i], a2)
            acc = _fma(dz[:, i, :, :, None], x[:, i, :, None, :], acc)
        p1, p2, ps = (a1[:, 0] + a1[:, 1]).astype(F), (a2[:, 0] + a2[:, 1]).astype(F), (acc[:, 0] + acc[:, 1]).astype(F)
        for ch in range(nch):
            A1[n] = (A1[n] + p1[ch]).astype(F)
            A2[n] = (A2[n] + p2[ch]).astype(F)
            S[n] = (S[n] + ps[ch]).astype(F)
    invL = F(1.0) / F(L_out)
    sw = np.zeros((8, C, Tn), dtype=F)
    sg = np.zeros((8, C), dtype=F)
    sb = np.zeros((8, C), dtype=F)
    for n in range(N):
        nl = n % 8
        X1 = x1[n][None, :]
        t2 = ((A1[n] * invL).astype(F)[:, None] * X1).astype(F)
        dd = (yx[n] - (mean[n][:, None] * X1).astype(F)).astype(F)
        t3 = (((A2[n] * invL).astype(F) * rstd[n]).astype(F)[:, None] * dd).astype(F)
        inner = ((S[n] - t2).astype(F) - t3).astype(F)
        sw[nl] = (sw[nl] + ((rstd[n] * ga).astype(F)[:, None] * inner).astype(F)).astype(F)
        sg[nl] = (sg[nl] + A2[n]).astype(F)
        sb[nl] = (sb[nl] + A1[n]).astype(F)
    out = {}
    for name, lanes, init in (("dw", sw, dw0), ("dgamma", sg, dgamma0), ("dbeta", sb, dbeta0)):
        a = np.zeros(lanes.shape[1:], dtype=F)
        for i in range(8):
            a = (a + lanes[i]).astype(F)
        out[name] = a if init is None else (_np(init).reshape(a.shape) + a).astype(F)
    out["_y"] = y_all
    return out


# ------------------------------------------------------------------------------------------------------------ shared cases
def make_case(kind: str, N: int, C_in: int, L_out: int, C: int, seed: int, k: int = 10, stride: int = 5, tail: int = 0, pad: int = 2) -> dict:
    """the operands of one forward call of one input kind: audio bf16 [N][C_in][L] with L = (L_out - 1) stride + k + tail, w bf16
    [C][C_in][k], gamma, beta, and geometry {k, stride, L_out, P = L_out + pad}
      offset    clips with a DC term, every fourth channel with all-positive taps: kappa = (s2 / L) / (var + eps) in the hundreds
      tiny      audio * 1e-3: the variance is below eps
      zero      clip 1 (clip 0 when N = 1) is silent
      constant  every clip one constant sample value
      highpass  the first three channels are difference filters on a smooth signal
      gamma0    every third gamma exactly 0
      tails     |beta| up to 6"""
    g = torch.Generator().manual_seed(seed)
    L = (L_out - 1) * stride + k + tail
    audio = torch.randn(N, C_in, L, generator=g)
    w = torch.randn(C, C_in, k, generator=g) * (2.0 / (C_in * k)) ** 0.5
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * torch.randn(C, generator=g)
    if kind == "offset":
        audio = 0.05 * audio + 1.0 + 0.25 * torch.arange(N).float()[:, None, None]
        w[::4] = w[::4].abs() + 0.05
    elif kind == "tiny":
        audio = audio * 1e-3
    elif kind == "zero":
        audio[min(1, N - 1)] = 0
    elif kind == "constant":
        audio = (0.3 + 0.2 * torch.arange(N).float())[:, None, None].expand(N, C_in, L).contiguous()
    elif kind == "highpass":
        t = torch.arange(L, dtype=torch.float64)
        sig = torch.stack([torch.sin(2 * np.pi * t / (900.0 + 37 * n)) + 0.5 * torch.sin(2 * np.pi * t / 210.0 + n) for n in range(N)])
        audio = (sig[:, None, :] + 1e-3 * audio.double()).float().expand(N, C_in, L).contiguous()
        w[:3] = 0
        w[0, 0, 4], w[0, 0, 5] = 1.0, -1.0
        w[1, 0, 3], w[1, 0, 4], w[1, 0, 5] = 1.0, -2.0, 1.0
        w[2, 0, :4] = torch.tensor([1.0, -3.0, 3.0, -1.0])
    elif kind == "gamma0":
        gamma[::3] = 0
    elif kind == "tails":
        beta = torch.linspace(-6, 6, C)[torch.randperm(C, generator=g)]
    elif kind != "randn":
        raise ValueError(kind)
    return dict(audio=audio.to(torch.bfloat16), w=w.to(torch.bfloat16), gamma=gamma, beta=beta, eps=1e-5,
                geometry=dict(k=k, stride=stride, L_out=L_out, P=L_out + pad), L=L, N=N, C_in=C_in, C=C, kind=kind)


def make_dact(case: dict, seed: int) -> torch.Tensor:
    """bf16 [N][P][C] output gradient, NaN on the padding rows (a launch must not read them)"""
    geo = case["geometry"]
    g = torch.Generator().manual_seed(seed)
    d = torch.full((case["N"], geo["P"], case["C"]), float("nan"))
    d[:, :geo["L_out"]] = torch.randn(case["N"], geo["L_out"], case["C"], generator=g)
    return d.to(torch.bfloat16)


def make_lists(counts: List[int], L_out: int, seed: int) -> List[List[int]]:
    """per clip `count` distinct ascending time steps; the first and the last step of the clip are in every list of two or more"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for cnt in counts:
        if cnt == 0:
            out.append([])
            continue
        perm = torch.randperm(L_out, generator=g)[:cnt].tolist()
        if cnt >= 2:
            perm[0], perm[1] = 0, L_out - 1
            perm = list(dict.fromkeys(perm))
            extra = [t for t in range(L_out) if t not in set(perm)]
            perm += extra[:cnt - len(perm)]
        out.append(sorted(perm))
    return out


def mask_unlisted(dact: torch.Tensor, lists: List[List[int]], L_out: int) -> torch.Tensor:
    """a copy of dact with every unlisted row NaN"""
    m = live_mask(dact.shape[0], L_out, lists)
    d = dact.clone()
    d[:, :L_out][~m] = float("nan")
    return d


# The shapes of tests/test_conv0_bounds_gpu.py; tests/test_conv0_reference_cpu.py runs the emulation over the same tables.
# forward: (N, C_in, C, L_out, pad = P - L_out, tail samples past the last tap, input kinds)
_PADS, _TAILS = (0, 2, 20), (0, 3, 7)
FWD_EDGES = [(3, 1, C, L_out, _PADS[(i + j) % 3], _TAILS[(i + 2 * j) % 3], KINDS)
             for j, C in enumerate((64, 48, 16)) for i, L_out in enumerate((1, 15, 16, 17, 255, 256, 257, 511, 512, 513))]
FWD_EDGES += [(3, 1, C, 510, 20, 3, ("randn", "offset")) for C in (64, 48, 16)]            # the padding crosses a 512 (and a 256) tile
FWD_TWO_CHANNELS = [(3, 2, C, L_out, 2, 3, ("randn", "offset", "highpass", "zero")) for C in (64, 80, 32) for L_out in (200, 513)]
FWD_WIDE = [(3, 1, 576, 33, 2, 0, ("randn", "offset", "tails")), (3, 1, 528, 33, 2, 0, ("randn", "offset", "tails")),
            (3, 1, 512, 300, 2, 0, ("randn", "offset"))]
FWD_LONG = [(2, 1, 64, 6430, 2, 4, ("randn", "highpass"))]
# long statistics chunks: (N, distinct clips, C_in, C, L_out): N = 1024 clips are the 8 distinct ones repeated
FWD_LONG_CHUNKS = [(1024, 8, 1, 64, 2100), (1024, 8, 2, 64, 1500)]
# backward, dense: (N, C_in, C, L_out, input kinds); every case runs into zeroed and into pre-filled accumulators
BWD_DENSE = [(1, 1, 16, 1, ("randn", "zero")), (8, 2, 64, 255, ("randn", "offset")), (9, 1, 576, 256, ("randn", "gamma0")),
             (17, 2, 16, 257, ("randn", "offset")), (17, 1, 64, 513, ("randn", "offset", "tails")), (9, 2, 576, 513, ("randn",)),
             (1, 1, 64, 257, ("randn", "constant")), (8, 1, 576, 1, ("randn", "tiny")), (9, 2, 64, 1, ("randn",)),
             (17, 1, 16, 255, ("highpass", "gamma0")), (1, 2, 576, 255, ("offset",)), (8, 1, 16, 513, ("randn", "tiny"))]
# backward, listed rows (mono, C = 64, L_out = 700, P = 702): (per-clip counts, max_rows - longest list, input kinds)
BWD_LISTED_L_OUT = 700
BWD_LISTED = [([0, 1, 255, 600], 0, ("randn", "offset")), ([256, 257, 513, 7], 0, ("randn", "offset")), ([0, 0, 300, 0], 0, ("randn",)),
              ([0, 1, 255, 600], 300, ("randn",)), ([256, 257, 513, 7], 1, ("offset",)),
              ([5, 0, 256, 700, 1, 300, 0, 12, 512, 255, 0, 257, 33, 600, 2, 0, 513], 0, ("randn", "offset")),
              ([5, 0, 256, 700, 1, 300, 0, 12, 512, 255, 0, 257, 33, 600, 2, 0, 513], 68, ("tails",))]
STRIDED = [(3, 64, 257), (3, 48, 257)]                    # (N, C, L_out) of the [N][2][L] batch run as two mono calls
