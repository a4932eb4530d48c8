"""Host-side dropout masks and a dropout layer for the oracle.  TEST INFRASTRUCTURE ONLY (a helper, not a test).

The engine's dropout masks come from a counter-based generator (wavjepa_amd/csrc/dropout_pieces.h): Philox4x32-10 keyed by the
64-bit seed, counter (group low, group high, site | layer << 8 | stack << 16, call), eight 16-bit draws per call, keep iff
draw >= thr = round(p * 65536).  Everything here rebuilds those masks bit for bit in numpy:

  philox4x32_10(counter, key)                         the generator itself (known answers in tests/test_dropout_cpu.py)
  row_keep(seed, call, stack, layer, site, M, N)      bool [M][N] of a row-major site (2 dropout1, 3 FFN, 4 dropout2)
  attn_keep(seed, call, stack, layer, B, H, Tq, Tk)   bool [B][H][Tq][Tk] of the attention site (1)
  thr_scale(p)                                        (thr, fp32 scale 65536 / (65536 - thr))

`dropout_layer` is the oracle's post-norm layer with the four masks as explicit arguments, written from the oracle's own `_lin`,
attention pieces and `_ln` (the dtype flow of oracle/jepa_oracle.py: probabilities rounded to bf16 BEFORE the mask in "bf16" mode,
as the kernel zeroes the rounded P; the survivors' scale on the output).  `install(monkeypatch, provider)` puts it in
J.post_norm_layer's place the way tests/prenorm_reference.py installs its layer; `provider(pre, B, T, D, H)` returns the four
masks in the ORACLE's dense layout or None (a layer without dropout: the teacher, a stack with p = 0).  `EngineMasks` is the
provider for a model step: it builds the launch-layout masks and, on a ragged step, scatters them into the dense layout through
the plan's row lists.

Attention against tests/attention_reference.py: `reference_fwd_drop` / `reference_bwd_drop` are that module's reference_fwd /
reference_bwd with P replaced by P o m in the P.V, dP and dV products and the outputs scaled; the bound terms are carried through the
same products and KAPPA is unchanged.  What the fp32 scale adds, derived here rather than by widening KAPPA: the kernel multiplies
the fp32 accumulator (O, dV) or dP by scale = fl32(65536 / (65536 - thr)) once -- one fp32 rounding of the quotient and one of the
product, each relative u32 = 2^-24, so 2 u32 |value| is added to the error term of out, dv and to ddP.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

from oracle import jepa_oracle as J

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
SITE_ATTN, SITE_RES1, SITE_FFN, SITE_RES2 = 1, 2, 3, 4
STACK = dict(enc=0, dec=1)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Arrays (or scalars) of uint32 values held in uint64 -> the four output words, uint64 arrays of 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3 = p1 & MASK32, p0 & MASK32
        c0, c2 = n0, n2
        k0 = (k0 + np.uint64(W0)) & MASK32
        k1 = (k1 + np.uint64(W1)) & MASK32
    return c0, c1, c2, c3


def thr_scale(p: float):
    p32 = float(np.float32(p))
    thr = min(65535, int(math.floor(p32 * 65536.0 + 0.5)))
    return thr, np.float32(65536.0) / np.float32(65536 - thr)


def stream_id(stack: int, layer: int, site: int) -> int:
    return site | layer << 8 | stack << 16


def group_draws(seed: int, call: int, sid: int, groups: np.ndarray) -> np.ndarray:
    """uint16-valued draws [..., 8] of the given group indices (uint64 array)."""
    g = np.asarray(groups, dtype=np.uint64)
    w = philox4x32_10(g & MASK32, g >> np.uint64(32), np.full(g.shape, sid, np.uint64), np.full(g.shape, call & 0xFFFFFFFF, np.uint64),
                      seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = np.empty(g.shape + (8,), dtype=np.uint32)
    for j in range(8):
        out[..., j] = ((w[j >> 1] >> np.uint64(16 * (j & 1))) & np.uint64(0xFFFF)).astype(np.uint32)
    return out


def row_keep(seed: int, call: int, stack: int, layer: int, site: int, M: int, N: int, p: float) -> np.ndarray:
    """bool [M][N]: element (row, col) is kept; group row * N / 8 + col / 8, draw col % 8."""
    assert N % 8 == 0
    thr, _ = thr_scale(p)
    d = group_draws(seed, call, stream_id(stack, layer, site), np.arange(M * (N // 8), dtype=np.uint64))
    return (d >= thr).reshape(M, N)


def attn_keep(seed: int, call: int, stack: int, layer: int, B: int, H: int, Tq: int, Tk: int, p: float, site: int = SITE_ATTN) -> np.ndarray:
    """bool [B][H][Tq][Tk]: group ((b H + h) 1024 + q) 128 + (k / 32) 4 + (k % 16) / 4, draw 4 ((k % 32) / 16) + k % 4."""
    thr, _ = thr_scale(p)
    k = np.arange(Tk)
    kg, kj = (k // 32) * 4 + (k % 16) // 4, 4 * ((k % 32) // 16) + k % 4
    ngk = int(kg.max()) + 1
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    q = np.arange(Tq, dtype=np.uint64)[None, :, None]
    groups = (bh * np.uint64(1024) + q) * np.uint64(128) + np.arange(ngk, dtype=np.uint64)[None, None, :]
    d = group_draws(seed, call, stream_id(stack, layer, site), groups)              # [BH][Tq][ngk][8]
    return (d[:, :, kg, kj] >= thr).reshape(B, H, Tq, Tk)


# ---------------------------------------------------------------------------------------------------------------- the oracle's layer
def attention_drop(qkv: torch.Tensor, nhead: int, key_mask: Optional[torch.Tensor], mode: str, m: Optional[torch.Tensor]) -> torch.Tensor:
    """J.attention with the probabilities multiplied by m ([B][H][T][T], keep * scale) behind their bf16 rounding."""
    B, T, D3 = qkv.shape
    D = D3 // 3
    hd = D // nhead
    cd = qkv.dtype if qkv.dtype == torch.float64 else torch.float32
    q, k, v = qkv.to(cd).view(B, T, 3, nhead, hd).permute(2, 0, 3, 1, 4)
    s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(hd))
    if key_mask is not None:
        s = s.masked_fill(key_mask[:, None, None, :], float("-inf"))
    p = torch.softmax(s, dim=-1)
    if mode == "bf16":
        p = p.to(torch.bfloat16).float()
    if m is not None:
        p = p * m.to(p.dtype)
    o = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, D)
    return o.to(torch.bfloat16) if mode == "bf16" else o


def _drop(x: torch.Tensor, m: Optional[torch.Tensor], mode: str) -> torch.Tensor:
    if m is None:
        return x
    y = x.float() * m.to(torch.float32) if x.dtype != torch.float64 else x * m.to(x.dtype)
    return y.to(torch.bfloat16) if mode == "bf16" else y


def _lin(x, w, b, mode: str):
    """J._lin; mode "fp64" (the comparison with torch's own layer, which J's fp32 casts would limit to 1e-7): the same product in fp64"""
    return F.linear(x.double(), w.double(), b.double()) if mode == "fp64" else J._lin(x, w, b, mode)


def _ln(x, w, b, eps: float, mode: str):
    return F.layer_norm(x.double(), (x.shape[-1],), w.double(), b.double(), eps) if mode == "fp64" else J._ln(x, w, b, eps)


def dropout_layer(P, pre: str, x: torch.Tensor, nhead: int, key_mask, mode: str, eps: float = 1e-6, masks: Optional[dict] = None):
    """J.post_norm_layer with masks = dict(attn, res1, ffn, res2) of keep * scale tensors in the layer's own shapes (None: no dropout)."""
    mk = masks or {}
    wide = (lambda t: t.double()) if mode == "fp64" else (lambda t: t.float())
    qkv = _lin(x, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"], mode)
    if mk.get("attn") is not None or mode == "fp64":
        a = attention_drop(qkv, nhead, key_mask, mode, mk.get("attn"))
    else:
        a = J.attention(qkv, nhead, key_mask, mode)
    sa = _drop(_lin(a, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"], mode), mk.get("res1"), mode)
    x = _ln(wide(x) + wide(sa), P[pre + "norm1.weight"], P[pre + "norm1.bias"], eps, mode)
    h = _lin(x, P[pre + "linear1.weight"], P[pre + "linear1.bias"], mode)
    h = _drop(F.gelu(h), mk.get("ffn"), mode)
    ff = _drop(_lin(h, P[pre + "linear2.weight"], P[pre + "linear2.bias"], mode), mk.get("res2"), mode)
    return _ln(wide(x) + wide(ff), P[pre + "norm2.weight"], P[pre + "norm2.bias"], eps, mode)


def install(monkeypatch, provider: Callable) -> None:
    """J.post_norm_layer <- dropout_layer with provider(pre, B, T, D, H) -> masks or None (see the module docstring)."""
    def layer(P, pre, x, nhead, key_mask, mode, eps=1e-6):
        return dropout_layer(P, pre, x, nhead, key_mask, mode, eps, provider(pre, x.shape[0], x.shape[1], x.shape[2], nhead))
    monkeypatch.setattr(J, "post_norm_layer", layer)


class EngineMasks:
    """provider for a model step: the masks the engine draws with (seed, call) for rates p = dict(enc=, dec=), in the oracle's dense
    [B][T] layout.  plan: the step's MaskPlan for a ragged step (None: the dense step, launch row = b T + t).  On a ragged step launch
    row r of the student is context row plan.keep[r], of the predictor visible row plan.dec_rows[r]; sequence b's query / key index is
    the position inside its packed sequence; the trimmed last predictor layer's sites 2-4 address the gathered target rows."""

    def __init__(self, seed: int, call: int, p: Dict[str, float], device, plan=None, tail: bool = False):
        self.seed, self.call, self.p, self.dev, self.plan, self.tail = seed, call, p, device, plan, tail
        self.n_layers: Dict[str, int] = {}

    def __call__(self, pre: str, B: int, T: int, D: int, H: int):
        stack = {"encoder.": "enc", "decoder.": "dec"}.get(pre.split("layers.")[0])
        if stack is None or not self.p.get(stack):
            return None
        layer, p = int(pre.split("layers.")[1].split(".")[0]), self.p[stack]
        s, sc = STACK[stack], float(thr_scale(p)[1])
        dev = self.dev
        if self.plan is None:
            row = lambda site, N: torch.from_numpy(row_keep(self.seed, self.call, s, layer, site, B * T, N, p)).reshape(B, T, N)
            attn = torch.from_numpy(attn_keep(self.seed, self.call, s, layer, B, H, T, T, p))
            return {k: (v.to(dev).float() * sc) for k, v in dict(attn=attn, res1=row(SITE_RES1, D), ffn=row(SITE_FFN, 4 * D),
                                                                   res2=row(SITE_RES2, D)).items()}
        plan = self.plan
        rows = (plan.keep if stack == "enc" else plan.dec_rows).long().cpu().numpy()          # dense (b T + t) of every launch row
        off = (plan.enc_off if stack == "enc" else plan.dec_off).long().cpu().numpy()
        R = rows.size
        b_of, pos = np.repeat(np.arange(B), np.diff(off)), np.arange(R) - np.repeat(off[:-1], np.diff(off))
        Lmax = int(np.diff(off).max())
        ak = attn_keep(self.seed, self.call, s, layer, B, H, Lmax, Lmax, p)                 # in sequence-local (q, k)
        attn = np.ones((B, H, T, T), dtype=bool)          # (key-masked or unused positions: the value is irrelevant)
        t_of = rows - b_of * T
        for b in range(B):
            tb = t_of[b_of == b]
            n = tb.size
            attn[b][:, tb[:, None], tb[None, :]] = ak[b][:, :n, :n]
        last = stack == "dec" and self.tail and layer == self._count(stack) - 1
        if last:                                          # sites 2-4 of the trimmed last layer: launch rows = the target rows
            rows = rows[plan.tgt_rows.long().cpu().numpy()]
            R = rows.size

        def row(site, N):
            out = np.ones((B * T, N), dtype=bool)
            out[rows] = row_keep(self.seed, self.call, s, layer, site, R, N, p)
            return torch.from_numpy(out).reshape(B, T, N)
        return {k: (v.to(dev).float() * sc) for k, v in dict(attn=torch.from_numpy(attn), res1=row(SITE_RES1, D), ffn=row(SITE_FFN, 4 * D),
                                                               res2=row(SITE_RES2, D)).items()}

    def _count(self, stack: str) -> int:
        return self.n_layers[stack]


# ---------------------------------------------------------------------------------------------------------------- single attention calls
def _mask_grid(o, keep_scale: torch.Tensor, b0: int, b1: int) -> torch.Tensor:
    """keep * scale [B][H][Tq][Tk] (sequence-local indices) -> the chunk's [n][H][Tm][Tm] fp64"""
    Tm = o.ix.Tm
    return keep_scale[b0:b1, :, :Tm, :Tm].double()


def core_drop(A, q, k, v, kval, qval, scale, hd, Mk, dO=None, O=None, dlse=None):
    """tests/attention_reference.py's core with P o Mk (Mk = keep * dropout scale) in P.V, dP and dV; see the module docstring."""
    U16, U32 = A.U16, A.U32
    T = q.shape[2]
    aq, ak, av = q.abs(), k.abs(), v.abs()
    S = (q @ k.transpose(-1, -2)) * scale
    e = hd * U32 * scale * (aq @ ak.transpose(-1, -2)) + 4 * U32 * (S.abs() + 1.0)
    S = S.masked_fill(~kval[:, None, None, :], float("-inf"))
    m = S.amax(-1, keepdim=True)
    dead = torch.isinf(m) | ~qval[:, None, :, None]
    m0 = torch.where(torch.isinf(m), torch.zeros_like(m), m)
    E = torch.exp(S - m0)
    ssum = E.sum(-1, keepdim=True)
    P = torch.where(dead, torch.zeros_like(E), E / torch.where(ssum > 0, ssum, torch.ones_like(ssum)))
    lsum = torch.log(torch.where(ssum > 0, ssum, torch.ones_like(ssum)))
    lse = torch.where(dead, torch.full_like(m0, float("inf")), m0 + lsum)
    e = e + 4 * U32 * m0.abs()
    ebar = (P * e).sum(-1, keepdim=True)
    PM = P * Mk
    r = {"out": PM @ v, "lse": lse[..., 0], "dead": dead[..., 0]}
    r["out_e"] = (PM * (U16 + e + ebar + T * U32)) @ av + 2 * U32 * r["out"].abs()
    r["lse_e"] = (ebar + T * U32 + 2 * U32 * (m0.abs() + lsum.abs() + torch.where(dead, torch.zeros_like(lse), lse).abs())
                  + 2.0 ** -22 * (1.0 + lsum.abs()))[..., 0]
    if dO is None:
        return r
    adO = dO.abs()
    dP = (dO @ v.transpose(-1, -2)) * Mk
    ddP = hd * U32 * (adO @ av.transpose(-1, -2)) * Mk + 2 * U32 * dP.abs()
    delta = (dO * O).sum(-1, keepdim=True)
    ddelta = hd * U32 * (adO * O.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    ep = e + dlse[..., None] + 2 * U32 * torch.where(dead, torch.zeros_like(lse), lse).abs() + T * U32 + U16
    W = dS.abs() * ep + P * scale * (ddP + ddelta)
    r["dq"], r["dq_e"] = dS @ k, W @ ak
    r["dk"], r["dk_e"] = dS.transpose(-1, -2) @ q, W.transpose(-1, -2) @ aq
    r["dv"] = PM.transpose(-1, -2) @ dO
    r["dv_e"] = (PM * ep).transpose(-1, -2) @ adO + 2 * U32 * r["dv"].abs()
    return r


def reference_fwd_drop(A, o, keep_scale: torch.Tensor, kappa: Optional[float] = None):
    kappa = A.KAPPA if kappa is None else kappa
    f, ix, dev = o.f, o.ix, o.device
    H, hd, D, R = f["H"], f["hd"], o.D, o.R
    ex = A.Expected()
    out, oe = torch.zeros(R, D, dtype=torch.float64, device=dev), torch.zeros(R, D, dtype=torch.float64, device=dev)
    lse, le = torch.zeros(R, H, dtype=torch.float64, device=dev), torch.zeros(R, H, dtype=torch.float64, device=dev)
    dead = torch.zeros(R, H, dtype=torch.bool, device=dev)
    for b0, b1 in A._chunks(f, ix.Tm):
        r = core_drop(A, A._gather(o, "qkv", b0, b1, 0), A._gather(o, "qkv", b0, b1, 1), A._gather(o, "qkv", b0, b1, 2), ix.kval[b0:b1],
                      ix.qval[b0:b1], 1.0 / math.sqrt(hd), hd, _mask_grid(o, keep_scale, b0, b1))
        A._scatter(o, out, r["out"], b0, b1)
        A._scatter(o, oe, r["out_e"], b0, b1)
        for dst, key in ((lse, "lse"), (le, "lse_e"), (dead, "dead")):
            A._scatter(o, dst, r[key][..., None], b0, b1)
    ex.ref["out"], ex.bound["out"] = out, torch.where(dead.repeat_interleave(hd, 1), torch.zeros_like(oe), A.out_bound(out, oe, kappa))
    ex.ref["lse"], ex.bound["lse"] = lse, kappa * le
    ex.dead = dead
    return ex


def reference_bwd_drop(A, o, fwd, keep_scale: torch.Tensor, kappa: Optional[float] = None):
    kappa = A.KAPPA if kappa is None else kappa
    f, ix, dev = o.f, o.ix, o.device
    H, hd, D, R = f["H"], f["hd"], o.D, o.R
    ex = A.Expected()
    ref = torch.zeros(R, 3 * D, dtype=torch.float64, device=dev)
    err = torch.zeros(R, 3 * D, dtype=torch.float64, device=dev)
    d = (o.lse_rows().double() - fwd.ref["lse"]).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    dl = torch.minimum(d, fwd.bound["lse"])
    for b0, b1 in A._chunks(f, ix.Tm):
        n = b1 - b0
        dlc = dl[ix.row[b0:b1].reshape(-1)].reshape(n, ix.Tm, H).permute(0, 2, 1)
        r = core_drop(A, A._gather(o, "qkv", b0, b1, 0), A._gather(o, "qkv", b0, b1, 1), A._gather(o, "qkv", b0, b1, 2), ix.kval[b0:b1],
                      ix.qval[b0:b1], 1.0 / math.sqrt(hd), hd, _mask_grid(o, keep_scale, b0, b1), dO=A._gather(o, "dout", b0, b1),
                      O=A._gather(o, "out", b0, b1), dlse=dlc)
        for j, key in enumerate(("dq", "dk", "dv")):
            A._scatter(o, ref[:, j * D:(j + 1) * D], r[key], b0, b1)
            A._scatter(o, err[:, j * D:(j + 1) * D], r[key + "_e"], b0, b1)
    bound = A.out_bound(ref, err, kappa)
    mk = torch.zeros(R, dtype=torch.bool, device=dev)
    mk[ix.row[ix.qval & ~ix.kval]] = True
    bound[:, D:] = torch.where(mk[:, None], torch.zeros_like(bound[:, D:]), bound[:, D:])
    bound[:, :D] = torch.where(fwd.dead.repeat_interleave(hd, 1), torch.zeros_like(bound[:, :D]), bound[:, :D])
    ex.ref["dqkv"], ex.bound["dqkv"] = ref, bound
    ex.masked_key_rows = mk
    return ex
