"""fp64 references, per-element error bounds, guards and mutations for the scene kernels `wj_rir_convolve` and `wj_snr_mix`
(csrc/scene.hip; test infrastructure, used by tests/test_scene_reference_cpu.py and tests/test_scene_bounds_gpu.py).

Every reference takes the inputs of one call as CPU tensors and returns {output: (fp64 reference, bound)}; `check` (norm_reference's)
requires every element finite and within its bound.  There is no norm of an output anywhere: the bounds below are norms of the INPUT
windows that feed one output block, so that a silent stretch has bound zero and must be exactly zero.  u = 2^-24.

RIR convolution (uniformly partitioned overlap-save, N = fft_size, Bk = N / 2, nb = ceil(T / Bk) blocks, P = ceil(L / Bk) partitions).
Output block j (samples [j Bk, (j + 1) Bk)) is the last Bk samples of ONE inverse FFT of sum_{p <= P' - 1} X[j - p] H[p], P' = min(P - 1, j) + 1,
X[i] the spectrum of x[(i - 1) Bk, (i + 1) Bk) and H[p] that of h[p Bk, (p + 1) Bk) | 0.  An fp32 FFT of length N returns a vector whose
error is ~ u log2(N) of its 2-norm, the product of two spectra carries both, and by Parseval and Cauchy-Schwarz a sample of the circular
convolution of a window with a partition is at most ||window||_2 ||partition||_2; hence, with a constant KF for the three transforms,
    bound[t] = KF u log2(N) sum_{p <= P' - 1} ||x[(j - p - 1) Bk, (j - p + 1) Bk)||_2 ||h[p Bk, (p + 1) Bk)||_2  +  u |ref[t]|     (store)
and in accumulate mode + u |prev[t] + ref[t]| (the addition).  KF is NOT fitted to the kernel: it is the smallest power of two at which
`emulate_rir_convolve` (torch fp32 FFTs in the kernel's block / partition structure, X[j - p] with H[p], accumulated over p in the
frequency domain) stays at or below 0.25 of the bound over every GPU case (tests/test_scene_reference_cpu.py asserts both halves of
that sentence); the factor 4 is room for what that emulation does not restate -- twiddle powers by squaring, sincospif, and the pair
packing (two real blocks per complex FFT).  That power is KF = 1/2: 0.214 of the bound there and 0.264 at KF = 1/4 (the worst is a
one-sample clip in accumulate mode, where the u |ref| terms are all there is; the other regimes sit at 0.002 - 0.11).
What the pair packing costs is measured by the emulation's second form (packed = True).  A member of a pair carries ~ u log2(N) of the
LOUDER member's size, which the local expression does not see: unscaled, a block fed by a one-tap partition alone behind a block a
thousand times louder (unit-impulse clip, L = 2 Bk + 1) stood at 1.49 of the bound, and a silent member was not silent.  The kernels
therefore keep an exactly silent member exactly silent (zero spectrum, zero block) and lift the quieter of two live members to its
partner's size by a power of two (pair_scales), and so does the second form: at most 0.19 of the bound.
The fp64 reference is the direct convolution (np.convolve), set exactly to zero where the bound is zero: an FFT reference leaves 1e-17
noise in silent stretches.

SNR mix.  Ex, En: sums of non-negative terms over the clipped window in the documented order (per chunk a strided fmaf chain per thread,
the wave butterfly, fold4; then the serial fold of the 64 chunk partials): relative error KAPPA u each (norm_reference.KAPPA; the
emulation of exactly that order measures its margin).  q = Ex / (En + 1e-9f) * exp10f(fl(-snr * 0.1f)), a = sqrtf(q):
    dq / q = KAPPA u + (KAPPA u En + u (En + 1e-9)) / (En + 1e-9) + u (division) + dg / g + u (product)
    dg / g = 6 u (exp10f: 3 ulp) + ln(10) |z| 2 u (z = -snr / 10: the rounded product and the rounded constant 0.1f)
    da / a = dq / (2 q) + u (sqrtf)             bound = |noise| a (da / a) + u |ref|  (one fmaf)
Ex = 0 gives a = 0 and out = source bit for bit: the bound is zero there.  Negative `start` is excluded: the kernel clips the window to
[0, T), the reference's slicing gives a negative start another meaning (EXCLUDED).

Mutations edit a copy of a correct output by the difference between a wrong and the right formula in fp64.  A mutation APPLIES to a
case when the wrong formula differs at all (convolution), or moves some gain by more than 2^-12 of itself on a channel whose noise is
not silent (SNR mix: the resolution the check claims, the same 2^-12 as the convolution's scaled result); where it applies `check` must
reject it.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.norm_reference import KAPPA, U, Pair, _butterfly, f64

F = np.float32
KF = 0.5                 # see the module docstring; pinned by tests/test_scene_reference_cpu.py
KF_MARGIN = 0.25
MIX_CHUNKS = 64
SNR_RESOLUTION = 2.0 ** -12

HANDLED = {
    "wj_rir_conv_args": {"x", "h", "y", "workspace", "h_stride_b", "h_stride_c", "B", "C", "T", "L", "accumulate", "fft_size"},
    "wj_snr_mix_args": {"source", "noise", "out", "snr", "start", "length", "workspace", "B", "C", "T"},
}
EXCLUDED = {
    "wj_snr_mix_args": {"start<0": "a VALUE, not a field: negative starts are not covered -- the kernel clips the window to [0, T), the "
                                   "reference's slicing counts a negative start from the end of the clip"},
}

# (B, C, T, L) of the GPU cases, by fft_size
CONV_CASES = {
    1024: [(2, 1, 1, 1), (1, 1, 511, 1), (1, 2, 512, 512), (1, 1, 513, 513), (1, 3, 1023, 1025), (2, 2, 1024, 1024), (1, 1, 1025, 2049),
           (1, 2, 1537, 1025), (3, 1, 2049, 1537), (1, 1, 100, 3000)],
    0: [(1, 1, 4095, 1), (1, 2, 4097, 4097), (1, 1, 8193, 4096), (1, 1, 100, 12289)],
}
EVERY_REGIME = {(1024, (1, 2, 1537, 1025)), (0, (1, 2, 4097, 4097))}
CONV_REGIMES = ("decay", "flat", "dc", "late", "zero", "h_tap0", "h_bk-1", "h_bk", "h_bk+1", "h_last", "x_imp0", "x_impbk")
SNR_CASES = [(1, 1, 1), (2, 2, 63), (1, 3, 64), (2, 1, 65), (1, 2, 257), (3, 2, 8191), (1, 1, 8193), (1, 1, 256 * 8192 + 1)]
SNR_WINDOWS = ("whole", "one", "past", "empty", "in_chunk", "seam")
SNR_DB = (-40.0, 0.0, 7.5, 40.0)
SNR_REGIMES = ("randn", "silent_source", "tiny_noise", "zero_noise_inside")


def fft_n(fft_size: int) -> int:
    return fft_size if fft_size else 8192


def conv_regimes(fft_size: int, case) -> Tuple[str, ...]:
    """every regime on the two cases the issue names, else two of the list in rotation (always one of the two Gaussian ones)"""
    if (fft_size, tuple(case)) in EVERY_REGIME:
        return CONV_REGIMES
    i = [c for cs in CONV_CASES.values() for c in cs].index(tuple(case))
    rest = CONV_REGIMES[2:]
    return (CONV_REGIMES[i % 2], rest[i % len(rest)], rest[(i + 5) % len(rest)])


def conv_runs():
    """(fft_size, case, regime, accumulate) of every checked GPU launch; the two cases that see every regime see both modes"""
    for fft, cases in CONV_CASES.items():
        for i, case in enumerate(cases):
            for k, regime in enumerate(conv_regimes(fft, case)):
                for acc in ((False, True) if (fft, case) in EVERY_REGIME else ((i + k) % 2 == 1,)):
                    yield fft, case, regime, acc


def snr_runs():
    """(case, regime, seed): six seeds give every b of a case every window kind; the 2^21-sample case (the apply grid at its cap) runs
    the whole-clip and the clipped window on Gaussian input"""
    for case in SNR_CASES[:-1]:
        for regime in SNR_REGIMES:
            for seed in range(6):
                yield case, regime, seed
    for seed in (0, 2):
        yield SNR_CASES[-1], "randn", seed


# ------------------------------------------------------------------------------------------------------------ convolution inputs
def conv_inputs(regime: str, B: int, C: int, T: int, L: int, N: int, seed: int, accumulate: bool = False) -> dict:
    """x [B][T], h [B][C][L] f32 (+ prev [B][C][T] Gaussian when accumulate)"""
    g = torch.Generator().manual_seed(seed)
    Bk = N // 2
    x = torch.randn(B, T, generator=g)
    decay = torch.exp(-torch.arange(L, dtype=torch.float32) / (0.3 * L + 1))
    h = torch.randn(B, C, L, generator=g)
    if regime != "flat":
        h = h * decay
    if regime == "dc":
        x = 1 + 0.01 * x
    elif regime == "late":
        x[:, :2 * Bk + 7] = 0
    elif regime == "zero":
        x = torch.zeros(B, T)
    elif regime.startswith("h_"):
        tap = {"h_tap0": 0, "h_bk-1": Bk - 1, "h_bk": Bk, "h_bk+1": Bk + 1, "h_last": L - 1}[regime]
        h = torch.zeros(B, C, L)
        h[:, :, min(tap, L - 1)] = 1.0
    elif regime.startswith("x_imp"):
        x = torch.zeros(B, T)
        x[:, min(0 if regime == "x_imp0" else Bk, T - 1)] = 1.0
    prev = torch.randn(B, C, T, generator=g) if accumulate else None
    return dict(x=x, h=h, prev=prev)


def _blocks(v: np.ndarray, n: int, Bk: int, lead: int, width: int) -> np.ndarray:
    """[..., len] -> [..., n, width]: block i = v[i Bk - lead, i Bk - lead + width), zeros outside"""
    pad = np.zeros(v.shape[:-1] + (lead + n * Bk + width,), dtype=v.dtype)
    pad[..., lead:lead + v.shape[-1]] = v
    return np.stack([pad[..., i * Bk:i * Bk + width] for i in range(n)], axis=-2)


# ------------------------------------------------------------------------------------------------------------ convolution reference
def _direct(x: np.ndarray, h: np.ndarray, T: int) -> np.ndarray:
    """[B][T], [B][C][L] fp64 -> [B][C][T]"""
    return np.stack([np.stack([np.convolve(x[b], h[b, c])[:T] for c in range(h.shape[1])]) for b in range(x.shape[0])])


def rir_convolve(x, h, fft_size: int = 0, prev=None, kf: float = KF) -> Dict[str, Pair]:
    """wj_rir_convolve: x [B][T], h [B][C][L] (ALREADY sliced out of its stack), prev [B][C][T] or None (accumulate)."""
    N = fft_n(fft_size)
    Bk = N // 2
    x64, h64 = f64(x).numpy(), f64(h).numpy()
    B, T = x64.shape
    C, L = h64.shape[1:]
    nb, P = -(-T // Bk), -(-L // Bk)
    xn = np.sqrt((_blocks(x64, nb, Bk, Bk, N) ** 2).sum(-1))                     # [B][nb]: ||x[(j - 1) Bk, (j + 1) Bk)||
    hn = np.sqrt((_blocks(h64, P, Bk, 0, Bk) ** 2).sum(-1))                      # [B][C][P]
    s = np.zeros((B, C, nb))
    for j in range(nb):
        for p in range(min(P - 1, j) + 1):
            s[:, :, j] += xn[:, None, j - p] * hn[:, :, p]
    blk = np.repeat(kf * U * math.log2(N) * s, Bk, axis=-1)[..., :T]
    ref = np.where(blk == 0, 0.0, _direct(x64, h64, T))
    bound = blk + U * np.abs(ref)
    if prev is not None:
        ref = ref + f64(prev).numpy()
        bound = bound + U * np.abs(ref)
    blk = torch.from_numpy(blk)
    return {"y": (torch.from_numpy(ref), torch.from_numpy(bound)), "_kf_term": (blk, blk)}


def _pair_scales(e0: np.ndarray, e1: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """pair_scales of csrc/scene.hip for arrays of pairs: [n] energies -> two [n][1] f32 powers of two that lift the quieter member"""
    s0, s1 = np.ones(e0.shape, dtype=F), np.ones(e0.shape, dtype=F)
    ok = (e0 > 0) & (e1 > 0) & np.isfinite(e0) & np.isfinite(e1)
    k = np.zeros(e0.shape, dtype=np.int64)
    k[ok] = np.trunc((np.frexp(e0[ok])[1] - np.frexp(e1[ok])[1]) / 2).astype(np.int64)
    s1[k > 0] = np.ldexp(F(1), np.minimum(k[k > 0], 60))
    s0[k < 0] = np.ldexp(F(1), np.minimum(-k[k < 0], 60))
    return s0[:, None], s1[:, None]


def emulate_rir_convolve(x, h, fft_size: int = 0, prev=None, packed: bool = False) -> np.ndarray:
    """The kernel's block / partition structure in torch fp32: spectra of the signal windows and of the zero-extended partitions, bins
    0 .. N/2, the products X[j - p] H[p] accumulated over p in the frequency domain, one inverse FFT per output block, its last Bk samples.
    This form sets KF.  packed = True restates the pair packing as well (two real blocks per complex FFT and the split of their spectra,
    two output blocks per inverse FFT as y0 + i y1, silent members kept exactly zero, the quieter member lifted by pair_scales): the more faithful form, used to explain what the
    kernel does beyond the first."""
    N = fft_n(fft_size)
    Bk, NB = N // 2, N // 2 + 1
    xf, hf = x.float().numpy(), h.float().numpy()
    B, T = xf.shape
    C, L = hf.shape[1:]
    nb, P = -(-T // Bk), -(-L // Bk)
    mirror = (-torch.arange(NB)) % N

    def spectra(blocks: np.ndarray) -> torch.Tensor:
        """[n][N] real -> [n][NB] complex64, members 2q and 2q + 1 through one FFT"""
        n = blocks.shape[0]
        if not packed:
            return torch.fft.rfft(torch.from_numpy(np.ascontiguousarray(blocks, dtype=F)))
        b = np.zeros((n + (n & 1), N), dtype=F)
        b[:n] = blocks
        s0, s1 = _pair_scales((b[0::2] ** 2).sum(1), (b[1::2] ** 2).sum(1))
        z = torch.fft.fft(torch.complex(torch.from_numpy(b[0::2] * s0), torch.from_numpy(b[1::2] * s1)))
        zk, zm = z[:, :NB], z[:, mirror].conj()
        first = torch.from_numpy(F(0.5) / s0) * (zk + zm)
        second = torch.complex(torch.tensor(0.0), torch.tensor(-1.0)) * torch.from_numpy(F(0.5) / s1) * (zk - zm)
        live = torch.from_numpy((b != 0).any(1)).reshape(-1, 2, 1)              # a silent member keeps an exactly zero spectrum
        return (torch.stack([first, second], 1) * live).reshape(-1, NB)[:n]

    out = np.zeros((B, C, T), dtype=F)
    for b in range(B):
        X = spectra(_blocks(xf[b], nb, Bk, Bk, N))
        for c in range(C):
            hb = np.zeros((P, N), dtype=F)
            hb[:, :Bk] = _blocks(hf[b, c], P, Bk, 0, Bk)
            H = spectra(hb)
            Y = torch.zeros(nb + (nb & 1), NB, dtype=torch.complex64)
            for p in range(min(P, nb)):
                Y[p:nb] = Y[p:nb] + X[:nb - p] * H[p]
            if not packed:
                out[b, c] = torch.fft.irfft(Y[:nb], n=N)[:, Bk:].reshape(-1)[:T].numpy()
                continue
            full = torch.cat([Y, Y[:, 1:NB - 1].flip(1).conj()], 1)              # Hermitian extension of both members
            e = (Y.real ** 2 + Y.imag ** 2).sum(1).numpy()
            s0, s1 = (torch.from_numpy(v) for v in _pair_scales(e[0::2], e[1::2]))
            z = torch.fft.ifft(full[0::2] * s0 + torch.complex(torch.tensor(0.0), torch.tensor(1.0)) * (full[1::2] * s1))
            live = (Y != 0).any(1).reshape(-1, 2, 1)                             # all products zero: the block is silence
            y = (torch.stack([z.real[:, Bk:] / s0, z.imag[:, Bk:] / s1], 1) * live).reshape(-1)[:T]
            out[b, c] = y.numpy()
    return out if prev is None else (prev.float().numpy() + out).astype(F)


# ------------------------------------------------------------------------------------------------------------ convolution mutations
def conv_mutations(got, x, h, fft_size: int, prev=None) -> List[Tuple[str, Optional[torch.Tensor]]]:
    """[(label, mutated fp64 output or None where the mutation does not apply)] of a correct output `got` [B][C][T]"""
    N = fft_n(fft_size)
    Bk = N // 2
    g = f64(got).clone()
    x64, h64 = f64(x).numpy(), f64(h).numpy()
    B, T = x64.shape
    C, L = h64.shape[1:]
    nb, P = -(-T // Bk), -(-L // Bk)
    direct = _direct(x64, h64, T)

    def moved(delta: np.ndarray):
        return g + torch.from_numpy(delta) if np.any(delta != 0) else None

    def part(p: int) -> np.ndarray:
        hp = np.zeros_like(h64)
        hp[..., p * Bk:(p + 1) * Bk] = h64[..., p * Bk:(p + 1) * Bk]
        return _direct(x64, hp, T)

    out = [("last partition dropped", moved(-part(P - 1))), ("first partition twice", moved(part(0)))]
    # one sample at a block seam takes position 0 of the circular convolutions (their wrap-around value) in place of position Bk
    seam = None
    if nb > 1:
        j = nb - 1
        xw = _blocks(x64, nb, Bk, Bk, N)                                          # [B][nb][N]
        wrap = np.zeros((B, C))
        for p in range(min(P - 1, j) + 1):
            hp = np.zeros((B, C, Bk))
            seg = h64[..., p * Bk:(p + 1) * Bk]
            hp[..., :seg.shape[-1]] = seg
            w = xw[:, j - p]                                                      # circ[0] = sum_k hp[k] w[(-k) mod N]
            wrap += hp[..., 0] * w[:, None, 0] + (hp[..., 1:] * w[:, None, :N - Bk:-1]).sum(-1)
        delta = np.zeros((B, C, T))
        delta[..., j * Bk] = wrap - direct[..., j * Bk]
        seam = moved(delta)
    out.append(("seam sample wrapped", seam))
    d0 = np.zeros((B, C, T))
    k = min(T, L)
    d0[..., :k] = -x64[:, None, :1] * h64[..., :k]
    out.append(("x[0] dropped", moved(d0)))
    swap = None
    if C >= 2:
        r = direct
        d = np.zeros_like(r)
        d[:, 0], d[:, 1] = r[:, 1] - r[:, 0], r[:, 0] - r[:, 1]
        swap = moved(d)
    out.append(("channel from h[c^1]", swap))
    out.append(("accumulate as overwrite", None if prev is None else moved(-f64(prev).numpy())))
    out.append(("scaled by 1 + 2^-12", moved(2.0 ** -12 * direct)))
    last = g.clone()
    last[..., T - 1] = float("nan") if prev is None else f64(prev)[..., T - 1]
    out.append(("sample T - 1 unwritten", last if prev is None or np.any(direct[..., T - 1] != 0) else None))
    return out


# ------------------------------------------------------------------------------------------------------------ SNR mix
def snr_inputs(regime: str, B: int, C: int, T: int, seed: int) -> dict:
    """source / noise [B][C][T], snr [B], start / length int32 [B]: window kind and SNR differ for every b"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, C, T, generator=g)
    n = 0.3 * torch.randn(B, C, T, generator=g)
    span = -(-T // MIX_CHUNKS)
    start, length, snr = [], [], []
    for b in range(B):
        kind = SNR_WINDOWS[(seed + b) % len(SNR_WINDOWS)]
        lo, ln = {"whole": (0, T), "one": (T // 2, 1), "past": (T - min(T, 5), 100), "empty": (T, 5),
                  "in_chunk": (span * min(3, MIX_CHUNKS - 1) % max(T, 1), max(1, span // 2)),
                  "seam": (max(0, min(T - 1, 2 * span) - 1), 3)}[kind]
        start.append(lo)
        length.append(ln)
        snr.append(SNR_DB[(seed + 3 * b) % len(SNR_DB)])
    start, length = torch.tensor(start, dtype=torch.int32), torch.tensor(length, dtype=torch.int32)
    for b in range(B):
        lo, hi = int(start[b]), min(T, int(start[b] + length[b]))
        if regime == "silent_source":
            s[b, :, lo:hi] = 0
        elif regime == "tiny_noise" and hi > lo:
            n[b, :, lo:hi] *= math.sqrt(1e-9 / max(float((n[b, :, lo:hi] ** 2).sum(-1).max()), 1e-30))
        elif regime == "zero_noise_inside":
            n[b, :, lo:hi] = 0
    return dict(source=s, noise=n, snr=torch.tensor(snr, dtype=torch.float32), start=start, length=length)


def _gain(s64, n64, snr, lo, hi, eps=float(F(1e-9)), div=10.0, per_bc=False, drop_last_chunk=False):
    """a [B][C] in fp64 (+ Ex, En); lo / hi [B] window bounds already clipped; per_bc: parameters read at index bc (mod B) instead of b"""
    B, C, T = s64.shape
    a, ex, en = np.zeros((B, C)), np.zeros((B, C)), np.zeros((B, C))
    span = -(-T // MIX_CHUNKS)
    for b in range(B):
        for c in range(C):
            i = (b * C + c) % B if per_bc else b
            l, h = int(lo[i]), int(hi[i])
            if drop_last_chunk:
                h = min(h, (MIX_CHUNKS - 1) * span)
            ex[b, c], en[b, c] = (s64[b, c, l:h] ** 2).sum(), (n64[b, c, l:h] ** 2).sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                a[b, c] = np.sqrt(np.float64(ex[b, c]) / np.float64(en[b, c] + eps) * 10.0 ** (-float(snr[i]) / div))
    return a, ex, en


def _window(start, length, T):
    st, ln = start.numpy().astype(np.int64), length.numpy().astype(np.int64)
    return np.maximum(st, 0), np.minimum(st + ln, T)


def snr_mix(source, noise, snr, start, length) -> Dict[str, Pair]:
    """wj_snr_mix: source / noise [B][C][T] f32, snr f32 [B], start / length int32 [B] (start >= 0)."""
    s64, n64 = f64(source).numpy(), f64(noise).numpy()
    T = s64.shape[-1]
    lo, hi = _window(start, length, T)
    a, ex, en = _gain(s64, n64, snr.numpy(), lo, hi)
    e = float(F(1e-9))
    z = np.abs(snr.numpy().astype(np.float64))[:, None] / 10.0
    dq = KAPPA * U + (KAPPA * U * en + U * (en + e)) / (en + e) + U + (6 * U + math.log(10.0) * z * 2 * U) + U
    da = a * (dq / 2 + U)
    ref = s64 + a[..., None] * n64
    bound = np.abs(n64) * da[..., None] + U * np.abs(ref)
    bound = np.where((a == 0)[..., None], 0.0, bound)
    return {"out": (torch.from_numpy(ref), torch.from_numpy(bound)), "a": (torch.from_numpy(a), torch.from_numpy(da))}


def _fma(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def emulate_snr_sums(v: np.ndarray, lo: int, hi: int) -> F:
    """sum of v[lo:hi]^2 ([T] f32) in the kernels' order: 64 chunks of span = ceil(T / 64); in a chunk thread i of 256 chains fmaf over
    t0 + i, t0 + i + 256, ...; wave butterflies, (w0 + w1) + (w2 + w3); then the 64 partials one after the other"""
    T = v.shape[0]
    span = -(-T // MIX_CHUNKS)
    its = -(-span // 256)
    seg = np.zeros((MIX_CHUNKS, its * 256), dtype=F)
    for ch in range(MIX_CHUNKS):
        t0, t1 = max(lo, ch * span), min(hi, (ch + 1) * span)
        if t1 > t0:
            seg[ch, :t1 - t0] = v[t0:t1]
    seg = seg.reshape(MIX_CHUNKS, its, 256)
    acc = np.zeros((MIX_CHUNKS, 256), dtype=F)
    for i in range(its):
        acc = _fma(seg[:, i], seg[:, i], acc)
    w = _butterfly(acc.reshape(MIX_CHUNKS, 4, 64))
    part = ((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F)
    tot = F(0)
    for ch in range(MIX_CHUNKS):
        tot = F(tot + part[ch])
    return tot


def emulate_snr_mix(source, noise, snr, start, length) -> Dict[str, np.ndarray]:
    """{"out", "a"}: the margin of the propagated part of the bound is measured on the gain a; the last term of the bound of `out`,
    u |ref|, is one correctly rounded fmaf and is attained at the bottom of a binade"""
    s, n = source.float().numpy(), noise.float().numpy()
    B, C, T = s.shape
    lo, hi = _window(start, length, T)
    out, gain = np.empty_like(s), np.zeros((B, C), dtype=F)
    for b in range(B):
        z = F(F(-snr.numpy()[b]) * F(0.1))
        g = F(10.0 ** np.float64(z))
        for c in range(C):
            ex, en = emulate_snr_sums(s[b, c], int(lo[b]), int(hi[b])), emulate_snr_sums(n[b, c], int(lo[b]), int(hi[b]))
            a = F(np.sqrt(np.float64(F(F(ex / F(en + F(1e-9))) * g))))
            out[b, c] = _fma(np.full(T, a, dtype=F), n[b, c], s[b, c])
            gain[b, c] = a
    return {"out": out, "a": gain}


def snr_mutations(got, source, noise, snr, start, length) -> List[Tuple[str, Optional[torch.Tensor]]]:
    """[(label, mutated fp64 output or None where the mutation does not apply)]"""
    g = f64(got)
    s64, n64 = f64(source).numpy(), f64(noise).numpy()
    B, C, T = s64.shape
    lo, hi = _window(start, length, T)
    sn = snr.numpy()
    a0, _, _ = _gain(s64, n64, sn, lo, hi)
    loud = np.abs(n64).max(-1) > 0
    lo1, hi1 = _window(start + 1, length, T)
    wrong = [("energies over the whole clip", _gain(s64, n64, sn, np.zeros(B, dtype=np.int64), np.full(B, T))[0]),
             ("window shifted by one", _gain(s64, n64, sn, lo1, hi1)[0]),
             ("snr[bc] / start[bc]", _gain(s64, n64, sn, lo, hi, per_bc=True)[0]),
             ("1e-9 omitted", _gain(s64, n64, sn, lo, hi, eps=0.0)[0]),
             ("last chunk's partial dropped", _gain(s64, n64, sn, lo, hi, drop_last_chunk=True)[0]),
             ("10^(-snr / 20)", _gain(s64, n64, sn, lo, hi, div=20.0)[0])]
    out = []
    for label, a1 in wrong:
        with np.errstate(invalid="ignore"):
            applies = loud & ~(np.abs(a1 - a0) <= SNR_RESOLUTION * a0)        # inf and nan gains apply
        if not applies.any():
            out.append((label, None))
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            out.append((label, g + torch.from_numpy((a1 - a0)[..., None] * n64)))
    return out
