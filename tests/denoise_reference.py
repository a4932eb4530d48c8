"""fp64 references, per-element error bounds and mutations for `wj_resample_fir`, `wj_mse_groups` (csrc/denoise.hip) and
`wj_crop_normalize_bf16` (csrc/misc.hip); test infrastructure, used by tests/test_denoise_reference_cpu.py and
tests/test_denoise_bounds_gpu.py.

Every reference takes the inputs of one call as CPU tensors and returns {output: (fp64 reference, bound)}; `check` (norm_reference's)
requires every element finite and within its bound; no norm anywhere.  u = 2^-24, KAPPA = norm_reference.KAPPA.

Resampler: the same-table reference (as tests/audio_prep_reference.py): the fp32 table the host built, applied in fp64,
    y[b][i nw + p] = sum_{k < taps} kernel[p][k] xpad[b][i orig + k],   xpad = x behind `width` zeros, zeros behind it.
The kernel is ONE chain of `taps` fmafs from zero: bound = (taps + 1) u sum_k |kernel[p][k] xpad[..]| (first order, worst case; zero
input gives bound zero and exactly zero output).

Grouped MSE: d = fl32(p - t) is exact to u |d|, so d^2 to 2 u d^2.  The sum of the non-negative d^2 runs in the documented order: up to
1024 partials of span = ceil(n / 1024) elements (per thread a strided fmaf chain, the wave butterfly, fold4), then a SERIAL fold of the
m non-empty partials:
    d loss[1 + g] / loss[1 + g] = 2 u + KAPPA u (inside a partial; the emulation measures its margin) + (m - 1) u (serial fold, worst
                                  case) + u (division by n)
    loss[0] = fmaf chain over g:  sum_g |w[g]| d loss[1 + g] + G u sum_g |w[g] loss[1 + g]|
    dpreds = c d, c = 2 w[g] / n * gscale (two roundings), d one, the product one: 5 u |ref| (one u spare).  preds = targets gives d = 0:
    loss and gradient exactly zero, bound zero.

Crop: mean and centred sum of squares in two passes (mean_sqdev: per thread a strided chain, block_sum), the propagation of
norm_reference's LayerNorm forward with the unbiased divisor and 1 / (std + 1e-5f):
    dmu = KAPPA u mean|x|        dc = u |c| + dmu        dvar = KAPPA u var + (2 dmu mean|c| + dmu^2) n / (n - 1) + u var
    dstd = dvar / (2 std) + u std        dinv / inv = (dstd + u (std + eps)) / (std + eps) + u
    dy = inv dc + |y| dinv / inv + u |y|        out: bf16_bound(y, dy)
A constant crop is exactly zero only where its value sums exactly in fp32 (the test uses -1.5); the bound above does not say so, the
GPU test asserts it on top.

Mutations edit a copy of a correct output by the difference between a wrong and the right formula in fp64 and return None where they
do not apply: where the wrong formula gives the same values (resampler), moves nothing by more than 2^-12 of itself (grouped MSE), or
moves nothing by more than two bf16 steps, 2^-6 of itself (crop).  Where a mutation applies, `check` must reject it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.norm_reference import KAPPA, U, Pair, _butterfly, bf16, bf16_bound, f64, mutate_truncate_bf16

F = np.float32
MSE_BLOCKS = 1024
RS_THREADS = 256
LDS_LIMIT = 64 * 1024
MSE_RESOLUTION = 2.0 ** -12
CROP_RESOLUTION = 2.0 ** -6

HANDLED = {
    "wj_resample_args": {"x", "kernel", "y", "B", "L_in", "L_out", "orig", "nw", "width", "taps"},
    "wj_mse_groups_args": {"preds", "targets", "w", "gscale", "loss", "dpreds", "workspace", "n", "G"},
    "wj_crop_args": {"src", "starts", "perm_inv", "out", "B", "S", "C", "L_full", "length"},
}
EXCLUDED: Dict[str, Dict[str, str]] = {}

KAISER_BEST = dict(lowpass_filter_width=64, rolloff=0.9475937167399596, resampling_method="sinc_interp_kaiser", beta=14.769656459379492)
# (orig_freq, new_freq, arguments of wavjepa_amd.resample.sinc_resample_kernel)
RATE_PAIRS = [
    (32000, 16000, KAISER_BEST),
    (48000, 32000, dict(lowpass_filter_width=6, resampling_method="sinc_interp_hann")),
    (16000, 24000, dict(lowpass_filter_width=16, resampling_method="sinc_interp_kaiser")),
    (8000, 16000, KAISER_BEST),
    (48000, 16000, KAISER_BEST),
]
LDS_PAIR = (48000, 5000, dict(lowpass_filter_width=6, resampling_method="sinc_interp_hann"))       # orig / nw = 48 / 5: 53 136 bytes of LDS
RESAMPLE_REGIMES = ("randn", "dc", "imp0", "implast", "zero")
FRAME_COUNTS = (255, 256, 257, 513)
MSE_N = (1, 255, 1023, 1024, 1025, 262145)
MSE_G = (1, 2, 4)
MSE_REGIMES = ("randn", "equal", "offset", "outlier")
CROP_CASES = [(1, 1, 1, 2, 2), (2, 3, 1, 5000, 1023), (2, 3, 1, 5000, 1024), (2, 3, 1, 5000, 1025), (2, 2, 2, 4100, 2049), (1, 4, 1, 40000, 32160)]
CROP_REGIMES = ("randn", "offset", "constant", "outlier")


# ------------------------------------------------------------------------------------------------------------ resampler
def table_for(orig_freq: int, new_freq: int, args: dict):
    """(fp32 table [nw][taps] as a tensor, width, orig, nw) as the product builds it for float32 waveforms"""
    from wavjepa_amd.resample import sinc_resample_kernel
    kern, width, orig, nw = sinc_resample_kernel(orig_freq, new_freq, dtype=torch.float32, **args)
    return torch.from_numpy(np.ascontiguousarray(kern)), width, orig, nw


def lds_bytes(orig: int, nw: int, width: int) -> int:
    """the entry's own formula"""
    taps = 2 * width + orig
    return (RS_THREADS * orig + taps + nw * taps) * 4


def smallest_refused_pair() -> Tuple[int, int, dict]:
    """the smallest orig : 1 (hann, lowpass_filter_width 6) whose table and window do not fit 64 KB by the entry's formula"""
    args = dict(lowpass_filter_width=6, resampling_method="sinc_interp_hann")
    for orig in range(2, 200):
        width = math.ceil(6 * orig / (0.99 * 1))
        if lds_bytes(orig, 1, width) > LDS_LIMIT:
            return orig, 1, args
    raise AssertionError("no refused pair below 200 : 1")


def out_len(L_in: int, orig: int, nw: int) -> int:
    return -(-nw * L_in // orig)


def resample_lengths(orig: int, nw: int, width: int) -> List[int]:
    """L_in in {1, width - 1, width, width + 1} and one L_in per frame count of FRAME_COUNTS: a partial last frame (L_out % nw != 0) at
    255 and 257 where the pair has one, a full one at 256 and 513"""
    out = [1, width - 1, width, width + 1]
    for fc in FRAME_COUNTS:
        fits = [L for L in range(1, fc * orig + orig + 1) if -(-out_len(L, orig, nw) // nw) == fc]
        want_partial = fc in (255, 257)
        pick = [L for L in fits if (out_len(L, orig, nw) % nw != 0) == want_partial] or fits
        out.append(pick[-1])
    return out


def resample_runs():
    """(table, width, orig, nw, B, L_in, regime) of every checked GPU launch: the five rate pairs, the table above 48 KB of LDS and
    the largest orig : 1 the entry accepts (65 488 bytes); Gaussian input at every length, the other regimes in rotation"""
    orig, nw, args = smallest_refused_pair()
    for i, (fo, fn, a) in enumerate(RATE_PAIRS + [LDS_PAIR, (orig - 1, nw, args)]):
        table, width, o, n = table_for(fo, fn, a)
        for k, L_in in enumerate(resample_lengths(o, n, width)):
            yield table, width, o, n, (3 if k == 4 else 1), L_in, "randn"
            yield table, width, o, n, 1, L_in, RESAMPLE_REGIMES[1 + (i + k) % 4]


def mse_runs():
    """(n, G, regime, gscale, with dpreds)"""
    for i, n in enumerate(MSE_N):
        for j, G in enumerate(MSE_G):
            for k, regime in enumerate(MSE_REGIMES):
                yield n, G, regime, (2.5 if (i + j + k) % 2 else None), (i + k) % 3 != 2


def crop_runs():
    """(B, S, C, L_full, length, regime, with a permutation)"""
    for i, (B, S, C, L_full, length) in enumerate(CROP_CASES):
        for k, regime in enumerate(CROP_REGIMES):
            yield B, S, C, L_full, length, regime, (i + k) % 2 == 0


def resample_input(regime: str, B: int, L_in: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L_in, generator=g)
    if regime == "dc":
        return torch.full((B, L_in), 0.625)
    if regime in ("imp0", "implast"):
        x = torch.zeros(B, L_in)
        x[:, 0 if regime == "imp0" else L_in - 1] = 1.0
    if regime == "zero":
        x = torch.zeros(B, L_in)
    return x


def _windows(x64: np.ndarray, frames: int, taps: int, orig: int, lead: int) -> np.ndarray:
    """[B][L_in] -> [B][frames][taps]: window i = xpad[i orig, i orig + taps) with `lead` zeros in front of x"""
    n = max((frames - 1) * orig + taps, lead + x64.shape[1])
    pad = np.zeros((x64.shape[0], n))
    pad[:, lead:lead + x64.shape[1]] = x64
    return np.lib.stride_tricks.sliding_window_view(pad, taps, axis=1)[:, ::orig][:, :frames]


def _apply(x, table, width: int, orig: int, nw: int, L_out: int, lead: Optional[int] = None, absolute: bool = False) -> np.ndarray:
    x64, t64 = f64(x).numpy(), f64(table).numpy()
    frames = -(-L_out // nw)
    win = _windows(x64, frames, t64.shape[1], orig, width if lead is None else lead)
    if absolute:
        win, t64 = np.abs(win), np.abs(t64)
    return np.einsum("bft,pt->bfp", win, t64).reshape(x64.shape[0], -1)[:, :L_out]


def resample_fir(x, table, width: int, orig: int, nw: int, L_out: int) -> Dict[str, Pair]:
    """wj_resample_fir: x [B][L_in] f32, table f32 [nw][2 width + orig]"""
    ref = _apply(x, table, width, orig, nw, L_out)
    bound = (table.shape[1] + 1) * U * _apply(x, table, width, orig, nw, L_out, absolute=True)
    return {"y": (torch.from_numpy(ref), torch.from_numpy(bound))}


def emulate_resample_fir(x, table, width: int, orig: int, nw: int, L_out: int) -> np.ndarray:
    """acc = fmaf(kernel[p][k], window[k], acc), k = 0 .. taps - 1, in fp32"""
    t32 = table.float().numpy()
    frames = -(-L_out // nw)
    win = _windows(x.float().numpy().astype(np.float64), frames, t32.shape[1], orig, width)      # fp32 values held in fp64
    acc = np.zeros((win.shape[0], frames, nw), dtype=F)
    for k in range(t32.shape[1]):
        acc = (t32[None, None, :, k].astype(np.float64) * win[:, :, None, k] + acc.astype(np.float64)).astype(F)
    return acc.reshape(win.shape[0], -1)[:, :L_out]


def resample_mutations(got, x, table, width: int, orig: int, nw: int, L_out: int) -> List[Tuple[str, Optional[torch.Tensor]]]:
    g = f64(got)
    right = _apply(x, table, width, orig, nw, L_out)

    def moved(wrong: np.ndarray):
        return g + torch.from_numpy(wrong - right) if np.any(wrong != right) else None

    out = [("phase p reads kernel[(p + 1) % nw]", moved(_apply(x, table.roll(-1, 0), width, orig, nw, L_out))),
           ("window shifted by one input sample", moved(_apply(x, table, width, orig, nw, L_out, lead=width + 1))),
           ("left padding width - 1", moved(_apply(x, table, width, orig, nw, L_out, lead=width - 1)))]
    last = g.clone()
    last[:, (-(-L_out // nw) - 1) * nw:] = float("nan")
    out.append(("last frame unwritten", last))
    return out


# ------------------------------------------------------------------------------------------------------------ grouped MSE
def mse_inputs(regime: str, G: int, n: int, seed: int) -> dict:
    """preds [G][n], targets [n], w [G] with a zero and a negative entry where G allows"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, generator=g)
    p = torch.randn(G, n, generator=g)
    if regime == "equal":
        p = t[None].repeat(G, 1)
    elif regime == "offset":
        t = 100 + t
        p = t[None] + 1e-3 * torch.randn(G, n, generator=g)
    elif regime == "outlier":
        p[:, n // 2] = 1e4
    w = torch.tensor([0.7, -0.3, 0.0, 1.25][:G])
    return dict(preds=p, targets=t, w=w)


def _mse_parts(n: int) -> Tuple[int, int]:
    span = -(-n // MSE_BLOCKS)
    return span, -(-n // span)


def mse_groups(preds, targets, w, gscale: Optional[float] = None, divisor: Optional[float] = None) -> Dict[str, Pair]:
    """wj_mse_groups: loss [1 + G] and dpreds [G][n]; gscale: the VALUE of gscale[0] (None: the pointer is NULL)"""
    p, t, w64 = f64(preds), f64(targets), f64(w)
    G, n = p.shape
    div = float(n) if divisor is None else divisor
    d = p - t
    l = (d * d).sum(1) / div
    _, m = _mse_parts(n)
    dl = l * (2 * U + KAPPA * U + (m - 1) * U + U)
    loss = torch.cat([(w64 * l).sum()[None], l])
    bl = torch.cat([((w64.abs() * dl).sum() + G * U * (w64 * l).abs().sum())[None], dl])
    c = 2.0 * w64 / div * (1.0 if gscale is None else float(F(gscale)))
    dp = c[:, None] * d
    return {"loss": (loss, bl), "dpreds": (dp, 5 * U * dp.abs())}


def _fold256(acc: np.ndarray) -> np.ndarray:
    """[..., 256] -> [...]: four wave butterflies, (w0 + w1) + (w2 + w3)"""
    w = _butterfly(acc.reshape(acc.shape[:-1] + (4, 64)))
    return ((w[..., 0] + w[..., 1]).astype(F) + (w[..., 2] + w[..., 3]).astype(F)).astype(F)


def emulate_mse_groups(preds, targets, w, gscale: Optional[float] = None) -> Dict[str, np.ndarray]:
    p, t, w32 = preds.float().numpy(), targets.float().numpy(), w.float().numpy()
    G, n = p.shape
    span, m = _mse_parts(n)
    its = -(-span // 256)
    d = (p - t[None]).astype(F)
    seg = np.zeros((G, MSE_BLOCKS, its * 256), dtype=F)
    for i in range(m):
        lo, hi = i * span, min(n, (i + 1) * span)
        seg[:, i, :hi - lo] = d[:, lo:hi]
    seg = seg.reshape(G, MSE_BLOCKS, its, 256)
    acc = np.zeros((G, MSE_BLOCKS, 256), dtype=F)
    for i in range(its):
        acc = (seg[:, :, i].astype(np.float64) ** 2 + acc.astype(np.float64)).astype(F)
    parts = _fold256(acc)
    loss = np.zeros(1 + G, dtype=F)
    total = F(0)
    for g in range(G):
        s = F(0)
        for i in range(MSE_BLOCKS):
            s = F(s + parts[g, i])
        loss[1 + g] = F(s / F(n))
        total = F(np.float64(w32[g]) * np.float64(loss[1 + g]) + np.float64(total))
    loss[0] = total
    c = ((F(2.0) * w32).astype(F) / F(n)).astype(F) * (F(1.0) if gscale is None else F(gscale))
    return {"loss": loss, "dpreds": (c.astype(F)[:, None] * d).astype(F)}


def _rel_moved(wrong: torch.Tensor, right: torch.Tensor, res: float) -> bool:
    return bool(((wrong - right).abs() > res * right.abs()).any())


def mse_mutations(got: dict, preds, targets, w, gscale: Optional[float]) -> List[Tuple[str, str, Optional[torch.Tensor]]]:
    """[(label, output, mutated or None)]; got: {"loss": [1 + G], "dpreds": [G][n] or None}"""
    right = mse_groups(preds, targets, w, gscale)
    G, n = preds.shape
    gl = f64(got["loss"])
    gd = None if got.get("dpreds") is None else f64(got["dpreds"])
    out = []

    def both(label, wrong):
        for k, g in (("loss", gl), ("dpreds", gd)):
            if g is None:
                continue
            ok = _rel_moved(wrong[k][0], right[k][0], MSE_RESOLUTION)
            out.append((label, k, g + (wrong[k][0] - right[k][0]) if ok else None))

    if n > 1:
        both("divides by n - 1", mse_groups(preds, targets, w, gscale, divisor=float(n - 1)))
    else:
        out.append(("divides by n - 1", "loss", torch.full_like(gl, float("inf"))))
    if G >= 2:
        swap = torch.arange(G) ^ 1
        both("w swapped between groups", mse_groups(preds, targets, w[swap], gscale))
        wrong = mse_groups(preds[swap], targets, w, gscale)
        if gd is not None:
            ok = _rel_moved(wrong["dpreds"][0], right["dpreds"][0], MSE_RESOLUTION)
            out.append(("dpreds[g] from preds[g^1]", "dpreds", gd + (wrong["dpreds"][0] - right["dpreds"][0]) if ok else None))
    if gscale is not None and gd is not None:
        wrong = mse_groups(preds, targets, w, None)
        ok = _rel_moved(wrong["dpreds"][0], right["dpreds"][0], MSE_RESOLUTION)
        out.append(("gscale ignored", "dpreds", gd + (wrong["dpreds"][0] - right["dpreds"][0]) if ok else None))
    span, m = _mse_parts(n)
    d = f64(preds) - f64(targets)
    tail = (d[:, (m - 1) * span:] ** 2).sum(1) / n
    wrong_l = right["loss"][0].clone()
    wrong_l[1:] -= tail
    wrong_l[0] -= (f64(w) * tail).sum()
    ok = m > 1 and _rel_moved(wrong_l, right["loss"][0], MSE_RESOLUTION)
    out.append(("last partial dropped", "loss", gl + (wrong_l - right["loss"][0]) if ok else None))
    return out


# ------------------------------------------------------------------------------------------------------------ crop
def crop_inputs(regime: str, B: int, S: int, C: int, L_full: int, length: int, seed: int, permute: bool) -> dict:
    """src [B][C][L_full], starts int32 [B][S] (0 and L_full - length among them), perm_inv int32 [B S] or None"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, C, L_full, generator=g)
    if regime == "offset":
        src = 100 + 1e-3 * src
    elif regime == "constant":
        src = torch.full((B, C, L_full), -1.5)
    starts = torch.randint(0, L_full - length + 1, (B, S), generator=g).to(torch.int32)
    starts[0, 0] = 0
    starts[-1, -1] = L_full - length
    if regime == "outlier":
        for b in range(B):
            for s in range(S):
                src[b, 0, int(starts[b, s]) + length // 2] = 1e3
    perm_inv = None
    if permute and B * S > 2:
        perm_inv = torch.roll(torch.arange(B * S), 1).to(torch.int32)          # a cycle: perm_inv is not its own inverse
    return dict(src=src, starts=starts, perm_inv=perm_inv)


def _crop_rows(src64: torch.Tensor, starts, length: int, shift: int = 0) -> torch.Tensor:
    """[B S][C length]: crop (b, s) of every channel; shift: start off by `shift` (clamped into the row)"""
    B, C, L_full = src64.shape
    rows = []
    for b in range(B):
        for s in range(starts.shape[1]):
            st = min(max(int(starts[b, s]) + shift, 0), L_full - length)
            rows.append(src64[b, :, st:st + length].reshape(-1))
    return torch.stack(rows)


def _place(rows: torch.Tensor, perm_inv) -> torch.Tensor:
    if perm_inv is None:
        return rows
    out = torch.empty_like(rows)
    out[perm_inv.long()] = rows
    return out


def _crop_y(x: torch.Tensor, how: str = "", C: int = 1) -> torch.Tensor:
    """the unrounded normalised rows under the right formula (how = "") or a wrong one"""
    if how == "per_channel":
        R = x.shape[0]
        return _crop_y(x.reshape(R * C, -1)).reshape(R, -1)
    n = x.shape[1]
    eps = float(F(1e-5))
    c = x - x.mean(1, keepdim=True)
    ss = (c * c).sum(1, keepdim=True)
    if how == "biased":
        return c / (torch.sqrt(ss / n) + eps)
    if how == "eps_inside":
        return c / torch.sqrt(ss / (n - 1) + eps)
    return c / (torch.sqrt(ss / (n - 1)) + eps)


def crop_normalize(src, starts, perm_inv, length: int) -> Dict[str, Pair]:
    """wj_crop_normalize_bf16: out [B S][C length] as fp64 values of bf16 numbers"""
    x = _crop_rows(f64(src), starts, length)
    n = x.shape[1]
    eps = float(F(1e-5))
    mu = x.mean(1, keepdim=True)
    c = x - mu
    var = (c * c).sum(1, keepdim=True) / (n - 1)
    std = torch.sqrt(var)
    inv = 1.0 / (std + eps)
    y = c * inv
    dmu = KAPPA * U * x.abs().mean(1, keepdim=True)
    dc = U * c.abs() + dmu
    dvar = KAPPA * U * var + (2 * dmu * c.abs().mean(1, keepdim=True) + dmu * dmu) * n / (n - 1) + U * var
    dstd = dvar / (2 * std).clamp_min(1e-300) + U * std
    dinv = (dstd + U * (std + eps)) / (std + eps) + U
    dy = inv * dc + y.abs() * dinv + U * y.abs()
    return {"out": (_place(bf16(y), perm_inv), _place(bf16_bound(y, dy), perm_inv)), "y": (_place(y, perm_inv), _place(dy, perm_inv))}


def _block_sum_1024(v: np.ndarray) -> np.ndarray:
    """[R][n] -> [R]: thread t of 1024 adds v[t], v[t + 1024], ... one by one; wave butterflies; the 16 waves in order"""
    R, n = v.shape
    its = -(-n // 1024)
    pad = np.zeros((R, its * 1024), dtype=F)
    pad[:, :n] = v
    pad = pad.reshape(R, its, 1024)
    acc = np.zeros((R, 1024), dtype=F)
    for i in range(its):
        acc = (acc + pad[:, i]).astype(F)
    waves = _butterfly(acc.reshape(R, 16, 64))
    tot = np.zeros(R, dtype=F)
    for wv in range(16):
        tot = (tot + waves[:, wv]).astype(F)
    return tot


def emulate_crop_normalize(src, starts, perm_inv, length: int) -> Dict[str, np.ndarray]:
    """the two-pass statistics in fp32 in mean_sqdev's order; "y" f32 in front of the bf16 rounding, "out" rounded"""
    x = _crop_rows(src.float(), starts, length).numpy()
    n = x.shape[1]
    mean = (_block_sum_1024(x) / F(n)).astype(F)[:, None]
    d = (x - mean).astype(F)
    q = _block_sum_1024((d.astype(np.float64) ** 2).astype(F))
    std = np.sqrt((q / F(n - 1)).astype(F).astype(np.float64)).astype(F)
    inv = (F(1.0) / (std + F(1e-5)).astype(F)).astype(F)[:, None]
    y = _place(torch.from_numpy((d * inv).astype(F)), perm_inv)
    return {"y": y.numpy(), "out": y.to(torch.bfloat16).float().numpy()}


def crop_mutations(got, src, starts, perm_inv, length: int, regime: str) -> List[Tuple[str, Optional[torch.Tensor]]]:
    """[(label, mutated fp64 output or None)] of a correct bf16 output `got` [B S][C length].  The truncating conversion, the biased
    divisor and the per-channel statistics apply to the regimes whose mean does not cancel (randn, outlier): at 100 + 1e-3 randn the
    bound of y itself, KAPPA u 100 against deviations of 1e-3, is some 5 % of a standard deviation and wider than what they move."""
    fine = regime in ("randn", "outlier")
    g = f64(got)
    src64 = f64(src)
    C = src64.shape[1]
    rows = _crop_rows(src64, starts, length)
    right = _crop_y(rows)

    def moved(wrong: torch.Tensor, inv=perm_inv):
        d = _place(wrong, inv) - _place(right, perm_inv)
        if not bool((d.abs() > CROP_RESOLUTION * _place(right, perm_inv).abs()).any()):
            return None
        return bf16(g + d)

    out = [("biased std", moved(_crop_y(rows, "biased")) if fine else None), ("eps inside the square root", moved(_crop_y(rows, "eps_inside"))),
           ("start off by one", moved(_crop_y(_crop_rows(src64, starts, length, shift=1))))]
    wrong_perm = None
    if perm_inv is not None:
        as_perm = torch.empty_like(perm_inv)
        as_perm[perm_inv.long()] = torch.arange(perm_inv.numel(), dtype=perm_inv.dtype)
        wrong_perm = moved(right, as_perm)
    out.append(("perm_inv applied as perm", wrong_perm))
    trunc = mutate_truncate_bf16(_place(right, perm_inv).float())
    out.append(("bf16 by truncation", trunc if fine and bool((trunc != g).any()) else None))
    out.append(("channels normalised separately", moved(_crop_y(rows, "per_channel", C)) if C > 1 and fine else None))
    return out
