"""fp64 reference and per-element bounds of the feed-forward activations of linear1's GEMM epilogue (wj_gemm_bf16_act,
include/wavjepa_hip_act.h): test infrastructure of tests/test_activation_cpu.py and tests/test_activation_ops_gpu.py.

Bound, in the form of tests/gemm_reference.py::epilogue_ref (h = bf16(v), dh = ulp_bf16(|v| + err) + err):
  e_act  = min(|act'(h)|  + A2 dh, A1) dh + APPROX |h|
  e_act' = min(|act''(h)| + A3 dh, A2) dh + APPROX (1 + |h|)
each wrapped in _out_bound (the output's own bf16 rounding).  A1..A3 = sup |act'|, |act''|, |act'''|, computed below on a grid.
ReLU has no bound: both outputs are exact functions of the bf16 h.

APPROX: the worst distance of an fp32 torch emulation of the kernel's own formula (csrc/common.h: silu_pk, gelu_tanh_pk) from fp64
over all finite bf16 inputs, in the units above (|h| for act, 1 + |h| for act'), times 4 because v_exp_f32 / v_rcp_f32 are 1-ulp
instructions and torch's fp32 exp / division are (nearly) correctly rounded.  Measured on the CPU (measure_approx(); the test pins
that each constant below is 4 x the measurement, rounded up by less than 10 %): silu 1.22e-7 -> 5e-7, gelu_tanh 3.16e-7 -> 1.3e-6,
beside gemm_reference.ERF_APPROX = 2e-7 for the erf-GELU.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Tuple

import torch

from tests.gemm_reference import _out_bound, bf16, ulp_bf16

KINDS = ("relu", "gelu_tanh", "silu")
C = math.sqrt(2.0 / math.pi)
A = 0.044715
APPROX = {"silu": 5e-7, "gelu_tanh": 1.3e-6}


def every_bf16() -> torch.Tensor:
    """all 65 536 bf16 bit patterns as float32 (NaN / inf included: filter with torch.isfinite)"""
    return (torch.arange(65536, dtype=torch.int32) << 16).view(torch.float32)


# ------------------------------------------------------------------------------------------------------------ fp64 functions
def _relu(h):
    return torch.where(h > 0, h, torch.zeros_like(h)), (h > 0).to(h.dtype), torch.zeros_like(h)


def _silu(h):
    s = torch.sigmoid(h)
    return h * s, s * (1 + h * (1 - s)), s * (1 - s) * (2 + h * (1 - 2 * s))


def _gelu_tanh(h):
    u = C * (h + A * h ** 3)
    t = torch.tanh(u)
    du = C * (1 + 3 * A * h * h)
    sech2 = 1 - t * t
    f = 0.5 * h * (1 + t)
    f1 = 0.5 * (1 + t) + 0.5 * h * sech2 * du
    f2 = sech2 * du + 0.5 * h * (-2 * t * sech2 * du * du + sech2 * 6 * A * C * h)
    # beyond saturation sech2 is exactly 0 in fp64 while du overflows nothing (|h| <= 3.4e38: h^2 ~ 1e77) -- 0 * finite
    return f, f1, f2


_FNS: Dict[str, Callable] = {"relu": _relu, "silu": _silu, "gelu_tanh": _gelu_tanh}


def act_fns(kind: str, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(act, act', act'') of a float64 tensor"""
    return _FNS[kind](h.double())


def _suprema(kind: str) -> Tuple[float, float, float]:
    x = torch.linspace(-12, 12, 480001, dtype=torch.float64)
    _, f1, f2 = act_fns(kind, x)
    f3 = (f2[2:] - f2[:-2]) / (x[2:] - x[:-2])
    return float(f1.abs().max()) * 1.001, float(f2.abs().max()) * 1.001, float(f3.abs().max()) * 1.01


SUP = {k: _suprema(k) for k in ("silu", "gelu_tanh")}      # (A1, A2, A3)


def act_ref(kind: str, v: torch.Tensor, err: torch.Tensor = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{"act": (fp64 reference, bound), "act1": (...)} for the fp64 pre-activation v = acc + bias with accumulation error err.
    Inputs below the smallest normal fp32 (bf16 subnormals) may reach the epilogue flushed to zero (the matrix pipe does not carry
    fp32 denormals): their dh is |v| itself."""
    v = v.double()
    err = torch.zeros_like(v) if err is None else err.double()
    h = bf16(v)
    f, f1, f2 = act_fns(kind, h)
    if kind == "relu":
        sub = ((v.abs() < 2.0 ** -126) & (v != 0)).double()                      # a flushed subnormal: act 0 for h, act' 0 for 1
        if not bool(err.any()):
            return {"act": (f, sub * v.abs()), "act1": (f1, sub)}
        return {"act": (f, _out_bound(f, ulp_bf16(v.abs() + err) + err)), "act1": (f1, sub)}
    dh = ulp_bf16(v.abs() + err) + err
    dh = torch.where(v.abs() < 2.0 ** -126, dh + v.abs(), dh)
    a1, a2, a3 = SUP[kind]
    e = torch.clamp(f1.abs() + a2 * dh, max=a1) * dh + APPROX[kind] * h.abs()
    e1 = torch.clamp(f2.abs() + a3 * dh, max=a2) * dh + APPROX[kind] * (1 + h.abs())
    return {"act": (f, _out_bound(f, e)), "act1": (f1, _out_bound(f1, e1))}


# ------------------------------------------------------------------------------------------------------------ fp32 emulation
def emulate_f32(kind: str, h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernel's own formula (csrc/common.h) in float32 torch ops, exp2 and reciprocal correctly rounded: (act, act') as float32"""
    x = h.float()
    one = torch.ones_like(x)
    if kind == "relu":
        return torch.where(x < 0, torch.zeros_like(x), x), (x > 0).float()
    if kind == "silu":
        e = torch.exp2(x * -1.44269504088896340736)
        s = one / (e + one)
        g = x * s
        return g, torch.addcmul(s, g, one - s)
    c2 = 2.0 * 0.79788456080286535588
    ke = -c2 * 1.44269504088896340736
    hc = x.clamp(-16.0, 16.0)
    q = hc * hc
    a = hc * (q * (ke * 0.044715) + ke)
    s = one / (torch.exp2(a) + one)
    w = hc * (q * (c2 * 0.134145) + c2)
    return x * s, torch.addcmul(s, s * (one - s), w)


def measure_approx(kind: str) -> float:
    """worst |emulation - fp64| over all finite bf16 inputs, in units of |h| (act) and 1 + |h| (act')"""
    v = every_bf16()
    v = v[torch.isfinite(v)]
    g, g1 = emulate_f32(kind, v)
    f, f1, _ = act_fns(kind, v)
    h = v.double().abs()
    nz = h > 0
    return max(float(((g.double() - f).abs()[nz] / h[nz]).max()), float(((g1.double() - f1).abs() / (1 + h)).max()))


# ------------------------------------------------------------------------------------------------------------ mutations
def erf_gelu(h: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    h = h.double()
    cdf = 0.5 * torch.erfc(-h / math.sqrt(2.0))
    return h * cdf, cdf + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def mutations(kind: str, h: torch.Tensor, act: torch.Tensor, act1: torch.Tensor):
    """(name, mutated act, mutated act') the way a subtly wrong epilogue would have stored them; h: the bf16 inputs as float64, act / act1:
    bf16 outputs.  Every one of them must fall outside act_ref's bounds somewhere."""
    r = lambda t: t.float().to(torch.bfloat16)
    if kind == "relu":
        z = (h == 0)
        if bool(z.any()):
            yield "derivative 1 at h == 0", act, torch.where(z, torch.ones_like(act1), act1)
    if kind == "silu":
        yield "silu' without the h (1 - s) term", act, r(torch.sigmoid(h.double()))
        yield "erf-GELU's derivative stored for a SiLU output", act, r(erf_gelu(h)[1])
    if kind == "gelu_tanh":
        g, g1 = erf_gelu(h)
        yield "tanh-GELU replaced by erf-GELU", r(g), r(g1)
    yield "act and act' swapped", act1, act


def check(kind: str, h: torch.Tensor, act: torch.Tensor, act1: torch.Tensor, err: torch.Tensor = None):
    """(failures, worst |got - ref| / bound) of bf16 outputs against act_ref (ReLU: exact equality of values)"""
    exp = act_ref(kind, h, err)
    fails, worst = [], 0.0
    for name, got in (("act", act), ("act1", act1)):
        if got is None:
            continue
        ref, bound = exp[name]
        g = got.double()
        d = (g - ref).abs()
        bad = ~torch.isfinite(g) | (d > bound)
        if bool(bad.any()):
            i = int(torch.nonzero(bad.reshape(-1))[0])
            fails.append(f"{kind} {name}: {int(bad.sum())} of {g.numel()} outside the bound (first: h {float(h.reshape(-1)[i]):.6g} got "
                         f"{float(g.reshape(-1)[i]):.6g} ref {float(ref.reshape(-1)[i]):.6g} bound {float(bound.reshape(-1)[i]):.3g})")
        ok = torch.isfinite(g) & (bound > 0)
        if bool(ok.any()):
            worst = max(worst, float((d[ok] / bound[ok]).max()))
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ oracle layer
def _act_fn(kind: str):
    import torch.nn.functional as F
    return {"gelu": F.gelu, "relu": F.relu, "silu": F.silu, "gelu_tanh": lambda h: F.gelu(h, approximate="tanh")}[kind]


def activation_layer(kind: str, pre_norm: bool = False):
    """A layer function for oracle.jepa_oracle in J.post_norm_layer's place (monkeypatch, as tests/prenorm_reference.py), written from
    the oracle's own _lin, attention and _ln -- the same dtype flow -- with the feed-forward activation `kind`, post- or pre-norm.
    tests/test_activation_cpu.py pins it to torch.nn.TransformerEncoderLayer(activation=...)."""
    from oracle import jepa_oracle as J
    act = _act_fn(kind)

    def post(P, pre, x, nhead, key_mask, mode, eps=1e-6):
        qkv = J._lin(x, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"], mode)
        a = J.attention(qkv, nhead, key_mask, mode)
        sa = J._lin(a, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"], mode)
        x = J._ln(x.float() + sa.float(), P[pre + "norm1.weight"], P[pre + "norm1.bias"], eps)
        h = act(J._lin(x, P[pre + "linear1.weight"], P[pre + "linear1.bias"], mode))
        ff = J._lin(h, P[pre + "linear2.weight"], P[pre + "linear2.bias"], mode)
        return J._ln(x.float() + ff.float(), P[pre + "norm2.weight"], P[pre + "norm2.bias"], eps)

    def pre_(P, pre, x, nhead, key_mask, mode, eps=1e-6):
        y = J._ln(x, P[pre + "norm1.weight"], P[pre + "norm1.bias"], eps)
        qkv = J._lin(y, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"], mode)
        a = J.attention(qkv, nhead, key_mask, mode)
        sa = J._lin(a, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"], mode)
        x = x.float() + sa.float()
        y = J._ln(x, P[pre + "norm2.weight"], P[pre + "norm2.bias"], eps)
        h = act(J._lin(y, P[pre + "linear1.weight"], P[pre + "linear1.bias"], mode))
        ff = J._lin(h, P[pre + "linear2.weight"], P[pre + "linear2.bias"], mode)
        return x + ff.float()
    return pre_ if pre_norm else post


def stack_layers(enc: str, dec: str, pre_norm: bool = False):
    """A layer function that switches by parameter prefix, for models whose stacks differ: `dec` for the predictor ("decoder."), `enc`
    for the student and its teacher."""
    fe, fd = activation_layer(enc, pre_norm), activation_layer(dec, pre_norm)

    def layer(P, pre, x, nhead, key_mask, mode, eps=1e-6):
        return (fd if pre.startswith("decoder.") else fe)(P, pre, x, nhead, key_mask, mode, eps)
    return layer
