"""fp64 reference, per-element error bound and region checks for single GEMM calls (test infrastructure; used by
tests/test_gemm_reference_cpu.py and tests/test_gemm_census_gpu.py).

A call is a plain dict of the fields of one `ops.gemm` / `ops.gemm_mxfp8` call or one problem of `ops.wgrad_grouped` (`call_fields`,
`wgrad_fields`).  `Operands` allocates every operand with a guard band behind it at the recorded address offset modulo 4 KiB, fills
the inputs with seeded data and the outputs with NaN (or, for += outputs, random f32); `reference` computes the fp64 result of every
output at the rounding points of include/wavjepa_hip.h together with a per-element bound (no norm anywhere); `check` holds what a
launch wrote against them: inside the output region every element finite and within its bound, outside it every byte unchanged.
The mutation helpers edit a copy of an output the way a subtly broken kernel would; `check` must reject each of them.

Bound (u = 2^-24, S = sum_k |alpha a_mk b_kn| in fp64):
  accumulation      e_acc = KAPPA u S + u (|bias| + |aux| + |C0|)          (each term only where that operand exists; KAPPA_FP8 for
                                                                            the MX fp8 GEMM)
  bf16 output       |got - ref| <= e (1 + 2^-8) + 2^-8 |ref|               (e: the propagated error in front of the rounding)
  bf16 intermediate h = bf16(acc (+ bias)): the kernel's h may sit one ulp of h away, dh = ulp(|v| + e_acc) + e_acc, propagated with
                    the local slope (|gelu'| <= 1.13, |gelu''| <= 0.8, |gelu'''| <= G3) or |aux|, plus the erf approximation (2e-7).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from wavjepa_amd._abi import ENUMS

U = 2.0 ** -24
KAPPA = 16.0              # fp32 accumulation: a k-ordered chain measures 1.3-6 u S up to K = 4096; 16 leaves room for split-K adds
# The MX fp8 GEMM's block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) does not sum like an fp32 k-ordered chain: the 4s-fp8 census
# (256 clips, K = 768 / 1536 / 3072) measured up to 5.6 x the KAPPA = 16 bound on its outputs, i.e. ~90 u S (the bf16 MFMA path of the
# same census stays within 1.0 x).  128 leaves 1.4 x over that measurement; the bf16 rounding term still dominates (2^-8 |ref| ~ 5e-3
# against 128 u S ~ 2e-4 at K = 768).
KAPPA_FP8 = 128.0
BF16_ROUND = 2.0 ** -8    # bf16 output rounding (<= half an ulp = 2^-8 |x|, taken as one ulp's worth with the binade edge)
GELU1 = 1.13              # max |gelu'|
GELU2 = 0.8               # max |gelu''| (2 phi(0) = 0.798)
ERF_APPROX = 2e-7         # the epilogues' fast erf: within 2e-7 |h| (tests/test_ops_gpu.py::test_gelu_epilogue_on_every_bf16_input)
GUARD_BYTES = 64 << 10
PAGE = 4096

EPI = {k[len("WJ_EPI_"):]: v for k, v in ENUMS.items() if k.startswith("WJ_EPI_")}
EPI_NAME = {v: k for k, v in EPI.items()}
# epilogues with a reference here; a header enum value missing from this set fails the census (coverage gate)
SUPPORTED_EPILOGUES = {"BF16", "BIAS_GELU2", "MUL_GELU_GRAD", "ADD_F32", "ATOMIC_F32", "CONV_GELU", "BIAS_GELU", "MUL_GELU_GRAD_Z",
                       "BF16_ADD_POS"}
FP8_EPILOGUES = {"BF16", "BIAS_GELU2", "BIAS_GELU"}
# the call fields the helper understands; a recorded call with any other field set fails the census
GEMM_KWARGS = {"A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "a_trans", "b_trans", "epilogue", "C2", "bias", "aux", "split_k",
               "seg_rows", "seg_valid", "alpha", "colsum", "rowmap", "workspace", "schedule", "persist_cus", "stream"}
FP8_KWARGS = {"A8", "B8", "scale_a", "scale_b", "C", "M", "N", "K", "lda", "ldb", "ldc", "ld_scale_a", "ld_scale_b", "epilogue", "C2",
              "bias", "q_out", "q_scales", "ld_q_scale", "stream"}


def _g3() -> float:
    x = np.linspace(-8, 8, 160001)
    return float(np.max(np.abs(np.exp(-x * x / 2) / math.sqrt(2 * math.pi) * (x ** 3 - 4 * x)))) * 1.01


GELU3 = _g3()             # max |gelu'''| (~0.78)


# ------------------------------------------------------------------------------------------------------------ call fields
def _ptr(x) -> int:
    if x is None:
        return 0
    return int(x) if isinstance(x, int) else int(x.data_ptr())


def call_fields(kw: dict, rowmap: Optional[np.ndarray] = None, entry: str = "gemm") -> dict:
    """The signature-relevant fields of an ops.gemm / ops.gemm_mxfp8 call (kw = its keyword arguments, A / B / C included).
    rowmap: the host copy of the gather list (M or K + 256 int32 entries)."""
    extra = set(k for k, v in kw.items() if v is not None) - (GEMM_KWARGS if entry == "gemm" else FP8_KWARGS)
    f = dict(entry=entry, unknown=tuple(sorted(extra)), M=int(kw["M"]), N=int(kw["N"]), K=int(kw["K"]), lda=int(kw["lda"]),
             ldb=int(kw["ldb"]), ldc=int(kw["ldc"]), epilogue=EPI_NAME.get(int(kw.get("epilogue", 0)), str(kw.get("epilogue"))),
             bias=kw.get("bias") is not None, C=kw.get("C") is not None, C2=kw.get("C2") is not None)
    names = ("A", "B", "C", "C2", "bias", "aux", "colsum") if entry == "gemm" else ("A8", "B8", "scale_a", "scale_b", "C", "C2", "bias",
                                                                                     "q_out", "q_scales")
    f["align"] = tuple((n, _ptr(kw.get(n)) % PAGE) for n in names if kw.get(n) is not None)
    if entry == "gemm":
        f.update(a_trans=int(kw.get("a_trans", 0)), b_trans=int(kw.get("b_trans", 0)), split_k=int(kw.get("split_k", 1)),
                 seg_rows=int(kw.get("seg_rows", 0)), seg_valid=int(kw.get("seg_valid", 0)), alpha=float(kw.get("alpha", 1.0)),
                 aux=kw.get("aux") is not None, colsum=kw.get("colsum") is not None, rowmap=rowmap,
                 workspace=kw.get("workspace") is not None, schedule=kw.get("schedule"), persist_cus=kw.get("persist_cus"))
    else:
        f.update(a_trans=0, b_trans=0, split_k=1, seg_rows=0, seg_valid=0, alpha=1.0, aux=False, colsum=False, rowmap=None,
                 workspace=False, schedule=None, persist_cus=None, ld_scale_a=int(kw["ld_scale_a"]), ld_scale_b=int(kw["ld_scale_b"]),
                 q_out=kw.get("q_out") is not None, ld_q_scale=int(kw.get("ld_q_scale") or 0))
    return f


def wgrad_fields(dY, X, gW, n_out: int, k_in: int, m_tok: int) -> dict:
    """One problem of ops.wgrad_grouped: gW[n_out][k_in] += dY[m_tok][n_out]^T X[m_tok][k_in] (col-form A and B, atomic f32)."""
    return dict(entry="wgrad", unknown=(), M=n_out, N=k_in, K=m_tok, lda=n_out, ldb=k_in, ldc=k_in, a_trans=1, b_trans=1,
                epilogue="ATOMIC_F32", split_k=0, seg_rows=0, seg_valid=0, alpha=1.0, bias=False, C=True, C2=False, aux=False,
                colsum=False, rowmap=None, workspace=False, schedule=None, persist_cus=None,
                align=tuple((n, _ptr(p) % PAGE) for n, p in (("A", dY), ("B", X), ("C", gW))))


def signature(f: dict) -> tuple:
    """Deduplication key: everything that selects a code path (the rowmap by its length only)."""
    keys = ("entry", "a_trans", "b_trans", "epilogue", "M", "N", "K", "lda", "ldb", "ldc", "split_k", "seg_rows", "seg_valid", "alpha",
            "bias", "C", "C2", "aux", "colsum", "workspace", "schedule", "persist_cus", "ld_scale_a", "ld_scale_b", "q_out", "ld_q_scale")
    return tuple((k, f.get(k)) for k in keys) + (("rowmap", None if f.get("rowmap") is None else len(f["rowmap"])),)


def describe(f: dict) -> str:
    lay = "NT"[f["a_trans"]] + "NT"[f["b_trans"]]            # bench.py's kernel names: N = row form, T = col form
    s = f"{f['entry']} {lay},{f['epilogue']} M={f['M']} N={f['N']} K={f['K']} lda={f['lda']} ldb={f['ldb']} ldc={f['ldc']}"
    if f["entry"] == "gemm" and f["split_k"] > 1:
        s += f" split={f['split_k']}"
    if f["seg_rows"]:
        s += f" seg={f['seg_rows']}/{f['seg_valid']}"
    if f["alpha"] != 1.0:
        s += f" alpha={f['alpha']:g}"
    for k in ("bias", "aux", "colsum", "workspace", "q_out"):
        if f.get(k):
            s += f" +{k}"
    if f.get("rowmap") is not None:
        s += f" rowmap[{len(f['rowmap'])}]"
    return s


def unsupported(f: dict) -> Optional[str]:
    """Why the helper has no reference for this call form (None: it has one)."""
    if f["unknown"]:
        return f"unknown fields {f['unknown']}"
    if f["epilogue"] not in SUPPORTED_EPILOGUES:
        return f"epilogue {f['epilogue']}"
    if f["entry"] == "gemm_mxfp8" and f["epilogue"] not in FP8_EPILOGUES:
        return f"fp8 epilogue {f['epilogue']}"
    if f.get("rowmap") is not None:
        form = (f["a_trans"], f["b_trans"], f["epilogue"])
        if form not in ((0, 1, "BF16"), (0, 1, "MUL_GELU_GRAD_Z"), (1, 1, "ATOMIC_F32")):
            return f"gather form {form}"
    if f["epilogue"] == "MUL_GELU_GRAD_Z" and f.get("rowmap") is None:
        return "MUL_GELU_GRAD_Z without a rowmap"
    return None


def _k_gather(f) -> bool:
    return f.get("rowmap") is not None and f["a_trans"] == 1


def _row_gather(f) -> bool:
    return f.get("rowmap") is not None and f["a_trans"] == 0


# ------------------------------------------------------------------------------------------------------------ extents
def out_dtypes(f: dict) -> Dict[str, torch.dtype]:
    e = f["epilogue"]
    d = {}
    if f["C"]:
        d["C"] = torch.float32 if e in ("ADD_F32", "ATOMIC_F32") else torch.bfloat16
    if f["C2"] and e in ("BIAS_GELU2", "CONV_GELU", "BF16_ADD_POS"):
        d["C2"] = torch.float32 if e == "BF16_ADD_POS" else torch.bfloat16
    return d


def extents(f: dict) -> Dict[str, Tuple[int, int, torch.dtype, int]]:
    """{operand: (lo, hi, dtype, ld)}: the element range [lo, hi) relative to the operand pointer that the call may touch, with the
    leading dimension used to size the guard band.  Row form [R][ld] with W columns: (R - 1) ld + W (overlapping windows included);
    gather forms use min / max of the rowmap (all K + 256 entries of the k-gather: its padding is read)."""
    M, N, K = f["M"], f["N"], f["K"]
    lda, ldb, ldc = f["lda"], f["ldb"], f["ldc"]
    rm = f.get("rowmap")
    ext = {}
    fp8 = f["entry"] == "gemm_mxfp8"
    if _k_gather(f):
        lo, hi = int(rm.min()), int(rm.max())
        ext["A"] = (lo * lda, hi * lda + M, torch.bfloat16, lda)
        ext["B"] = (lo * ldb, hi * ldb + N, torch.bfloat16, ldb)
    elif _row_gather(f):
        lo, hi = int(rm.min()), int(rm.max())
        ext["A"] = (lo * lda, hi * lda + K, torch.bfloat16, lda)
        ext["B"] = (0, (K - 1) * ldb + N, torch.bfloat16, ldb)
    else:
        adt = torch.uint8 if fp8 else torch.bfloat16
        ext["A"] = (0, (K - 1) * lda + M, adt, lda) if f["a_trans"] else (0, (M - 1) * lda + K, adt, lda)
        ext["B"] = (0, (K - 1) * ldb + N, adt, ldb) if f["b_trans"] else (0, (N - 1) * ldb + K, adt, ldb)
    crange = (int(rm.min()) * ldc, int(rm.max()) * ldc + N) if _row_gather(f) else (0, (M - 1) * ldc + N)
    for name, dt in out_dtypes(f).items():
        ext[name] = crange + (dt, ldc)
    if f["bias"]:
        ext["bias"] = (0, N, torch.float32, N)
    if f["aux"]:
        e = f["epilogue"]
        if e == "BF16_ADD_POS":
            ext["aux"] = (0, f["seg_rows"] * N, torch.float32, N)
        else:
            ext["aux"] = crange + (torch.float32 if e == "ADD_F32" else torch.bfloat16, ldc)
    if f["colsum"]:
        ext["colsum"] = (0, N, torch.float32, N)
    if fp8:
        ext["scale_a"] = (0, (K // 128) * f["ld_scale_a"] + 256, torch.int32, f["ld_scale_a"])
        ext["scale_b"] = (0, (K // 128) * f["ld_scale_b"] + 256, torch.int32, f["ld_scale_b"])
        if f["q_out"]:
            ext["q_out"] = (0, (M - 1) * ldc + N, torch.uint8, ldc)
            ext["q_scales"] = (0, (N // 128) * f["ld_q_scale"] + 256, torch.int32, f["ld_q_scale"])
    return ext


def _nan_bits(dt: torch.dtype) -> int:
    return {torch.bfloat16: 0x7FC0, torch.float32: 0x7FC00000, torch.uint8: 0x7F, torch.int32: 0x7FC00000}[dt]


def _ibits(t: torch.Tensor) -> torch.Tensor:
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32}[t.dtype])


class Buf:
    """One operand: a flat allocation [front guard | placement shift | extent | guard band], `p` = index of the operand pointer."""

    def __init__(self, lo: int, hi: int, dt: torch.dtype, ld: int, offset: Optional[int], device):
        es = torch.tensor([], dtype=dt).element_size()
        guard = GUARD_BYTES + 512 * max(ld, 1) * es                     # a tail tile's rows read behind the last row stay inside
        n = PAGE // es + PAGE // es + (hi - lo) + guard // es
        self.t = torch.empty(n, dtype=dt, device=device)
        base = self.t.data_ptr() + PAGE + (-lo) * es                  # pointer with no placement shift
        shift = 0 if offset is None else (offset - base) % PAGE
        assert shift % es == 0
        self.p = PAGE // es + shift // es + (-lo)
        self.lo, self.hi, self.dt, self.es = lo, hi, dt, es
        _ibits(self.t).fill_(_nan_bits(dt) if dt in (torch.bfloat16, torch.float32) else 0)

    @property
    def ptr(self) -> int:
        return self.t.data_ptr() + self.p * self.es

    def rows(self, r0: int, nrows: int, width: int, ld: int, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[nrows][width] view of rows r0.. (stride ld) relative to the operand pointer."""
        t = self.t if t is None else t
        return t.as_strided((nrows, width), (ld, 1), self.p + r0 * ld)


# ------------------------------------------------------------------------------------------------------------ operands
def _gen(seed: int, device) -> torch.Generator:
    return torch.Generator(device=device).manual_seed(seed)


def _randn(n: int, g, scale: float = 1.0) -> torch.Tensor:
    return torch.randn(n, generator=g, dtype=torch.float32, device=g.device) * scale


def quantize_mxfp8_torch(x: torch.Tensor, M: int, K: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The documented rule of wj_quantize_mxfp8 on a [M][K] bf16 matrix: (e4m3 bytes [M][K], exponents [M][K/32] as int)."""
    xf = x.float().reshape(M, K // 32, 32)
    amax = xf.abs().amax(-1)
    s = torch.where(amax > 0, torch.ceil(torch.log2(amax / 448.0)), torch.zeros_like(amax))
    q = (xf * torch.exp2(-s)[..., None]).reshape(M, K).to(torch.float8_e4m3fn).view(torch.uint8)
    return q, s.to(torch.int32) + 127


def pack_scales(e: torch.Tensor, ld: int, out: torch.Tensor, offset: int) -> None:
    """exponent bytes [rows][K/32] -> dwords [K/128][ld] (byte b of dword (kt, r) = block 4 kt + b of row r) written into out"""
    rows, nb = e.shape
    b = e.reshape(rows, nb // 4, 4).permute(1, 0, 2).to(torch.int64)
    dw = (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16) | (b[..., 3] << 24))
    dw = torch.where(dw >= 2 ** 31, dw - 2 ** 32, dw).to(torch.int32)
    out.as_strided((nb // 4, rows), (ld, 1), offset).copy_(dw)


class Operands:
    """Every operand of one call, allocated, placed and filled with seeded synthetic data."""

    def __init__(self, f: dict, device, seed: int = 0, a_scale: float = 1.0, b_scale: float = 0.05):
        self.f, self.device = f, device
        align = dict(f.get("align", ()))
        ext = extents(f)
        if f["entry"] == "gemm_mxfp8":                                 # the pointers were recorded under the fp8 names
            align = dict(align, A=align.get("A8"), B=align.get("B8"))
        self.b = {n: Buf(lo, hi, dt, ld, align.get(n), device) for n, (lo, hi, dt, ld) in ext.items()}
        self.rowmap = None if f.get("rowmap") is None else torch.as_tensor(np.asarray(f["rowmap"], dtype=np.int32)).to(device)
        self.rm_long = None if self.rowmap is None else self.rowmap.long()
        g = _gen(seed, device)
        M, N, K = f["M"], f["N"], f["K"]
        e = f["epilogue"]
        if f["entry"] == "gemm_mxfp8":
            for name, rows, ld, sname, lds, sc in (("A", M, f["lda"], "scale_a", f["ld_scale_a"], a_scale),
                                                   ("B", N, f["ldb"], "scale_b", f["ld_scale_b"], b_scale)):
                x = _randn(rows * K, g, sc).to(torch.bfloat16).reshape(rows, K)
                q, ex = quantize_mxfp8_torch(x, rows, K)
                self.b[name].rows(0, rows, K, ld).copy_(q)
                sb = self.b[sname]
                sb.t[sb.p:sb.p + sb.hi].zero_()
                pack_scales(ex, lds, sb.t, sb.p)
        else:
            self._fill_matrix("A", a_scale, g)
            self._fill_matrix("B", b_scale, g)
        if f["bias"]:
            self.b["bias"].t[self.b["bias"].p:][:N].copy_(_randn(N, g))
        if f["aux"]:
            a = self.b["aux"]
            if e == "BF16_ADD_POS":
                a.t[a.p:a.p + a.hi].copy_(_randn(a.hi, g, 0.25))
            elif e == "ADD_F32":
                self.set_region("aux", _randn(M * N, g).reshape(M, N))
            elif e == "MUL_GELU_GRAD":                                  # gelu'(h) of a random bf16 h
                h = _randn(M * N, g, 1.5).to(torch.bfloat16).double()
                self.set_region("aux", gelu1(h).reshape(M, N).to(torch.bfloat16))
            else:                                                       # MUL_GELU_GRAD_Z: a bf16 pre-activation z
                self.set_region("aux", _randn(M * N, g, 1.5).to(torch.bfloat16).reshape(M, N))
        self._seed_out = seed + 7919

    def _fill_matrix(self, name: str, scale: float, g) -> None:
        f, b = self.f, self.b[name]
        M, N, K = f["M"], f["N"], f["K"]
        ld = f["lda"] if name == "A" else f["ldb"]
        trans = f["a_trans"] if name == "A" else f["b_trans"]
        width = {"A": M if trans else K, "B": N if trans else K}[name]
        if width > ld:                              # overlapping windows (implicit-GEMM convs, tap gathers): the whole extent is data
            b.t[b.p + b.lo:b.p + b.hi].copy_(_randn(b.hi - b.lo, g, scale).to(torch.bfloat16))
            return
        if (_row_gather(f) and name == "A") or (_k_gather(f)):
            rm = self.rm_long[:f["M"]] if _row_gather(f) else self.rm_long[:K]
            lo = int(rm.min())
            rows = b.rows(lo, int(rm.max()) - lo + 1, width, ld)
            vals = _randn(rm.numel() * width, g, scale).to(torch.bfloat16).reshape(-1, width)
            rows[rm - lo] = vals
            return
        R, W = (K, M) if (name == "A" and trans) else (M, K) if name == "A" else (K, N) if trans else (N, K)
        b.rows(0, R, W, ld).copy_(_randn(R * W, g, scale).to(torch.bfloat16).reshape(R, W))

    def _out_region(self, name: str, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[M][N] region of an output-shaped operand (C, C2, aux of C's layout, q_out) as a view, or a gathered copy for row gathers
        (use set_region to write it)."""
        f, b = self.f, self.b[name]
        if _row_gather(f):
            lo = int(self.rm_long.min())
            return b.rows(lo, int(self.rm_long.max()) - lo + 1, f["N"], f["ldc"], t)[self.rm_long[:f["M"]] - lo]
        return b.rows(0, f["M"], f["N"], f["ldc"], t)

    def region(self, name: str, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        return self._out_region(name, t)

    def set_region(self, name: str, vals: torch.Tensor, t: Optional[torch.Tensor] = None) -> None:
        f, b = self.f, self.b[name]
        if _row_gather(f):
            lo = int(self.rm_long.min())
            b.rows(lo, int(self.rm_long.max()) - lo + 1, f["N"], f["ldc"], t)[self.rm_long[:f["M"]] - lo] = vals
        else:
            b.rows(0, f["M"], f["N"], f["ldc"], t).copy_(vals)

    def reset_outputs(self, seed: Optional[int] = None) -> None:
        """Every output allocation NaN; += outputs (ATOMIC_F32 C, colsum) start from random f32 inside their region."""
        f = self.f
        g = _gen(self._seed_out if seed is None else seed, self.device)
        for name in list(out_dtypes(f)) + (["colsum"] if f["colsum"] else []) + (["q_out", "q_scales"] if f.get("q_out") else []):
            b = self.b[name]
            _ibits(b.t).fill_(_nan_bits(b.dt) if b.dt != torch.uint8 else 0x7F)
        if f["epilogue"] == "ATOMIC_F32":
            self.set_region("C", _randn(f["M"] * f["N"], g).reshape(f["M"], f["N"]))
        if f["colsum"]:
            cs = self.b["colsum"]
            cs.t[cs.p:cs.p + f["N"]].copy_(_randn(f["N"], g))

    def snapshot(self) -> Dict[str, torch.Tensor]:
        names = list(out_dtypes(self.f)) + (["colsum"] if self.f["colsum"] else []) + (["q_out", "q_scales"] if self.f.get("q_out") else [])
        return {n: self.b[n].t.clone() for n in names}

    def outputs(self) -> Dict[str, torch.Tensor]:
        return {n: self.b[n].t for n in self.snapshot_names()}

    def snapshot_names(self) -> List[str]:
        return list(out_dtypes(self.f)) + (["colsum"] if self.f["colsum"] else []) + (["q_out", "q_scales"] if self.f.get("q_out") else [])

    def kwargs(self) -> dict:
        """Keyword arguments for the ops entry point (pointers as ints)."""
        f, b = self.f, self.b
        p = lambda n: b[n].ptr if n in b else None
        kw = dict(M=f["M"], N=f["N"], K=f["K"], lda=f["lda"], ldb=f["ldb"], ldc=f["ldc"], epilogue=EPI[f["epilogue"]])
        if f["entry"] == "gemm_mxfp8":
            kw.update(A8=p("A"), B8=p("B"), scale_a=p("scale_a"), scale_b=p("scale_b"), C=p("C"), C2=p("C2"), bias=p("bias"),
                      ld_scale_a=f["ld_scale_a"], ld_scale_b=f["ld_scale_b"])
            if f["q_out"]:
                kw.update(q_out=p("q_out"), q_scales=p("q_scales"), ld_q_scale=f["ld_q_scale"])
            return kw
        kw.update(A=p("A"), B=p("B"), C=p("C"), C2=p("C2"), bias=p("bias"), aux=p("aux"), colsum=p("colsum"),
                  a_trans=f["a_trans"], b_trans=f["b_trans"], split_k=f["split_k"], seg_rows=f["seg_rows"], seg_valid=f["seg_valid"],
                  alpha=f["alpha"], rowmap=self.rowmap)
        return kw

    # ---- logical operands in fp64
    def a_block(self, m0: int, m1: int, k0: int, k1: int) -> torch.Tensor:
        f, b = self.f, self.b["A"]
        M, K, lda = f["M"], f["K"], f["lda"]
        if f["entry"] == "gemm_mxfp8":
            return self._dequant("A", "scale_a", f["ld_scale_a"], m0, m1, k0, k1)
        if _row_gather(f):
            rm = self.rm_long[m0:m1]
            lo = int(rm.min())
            return b.rows(lo, int(rm.max()) - lo + 1, K, lda)[rm - lo][:, k0:k1].double()
        if _k_gather(f):
            rm = self.rm_long[k0:k1]
            lo = int(rm.min())
            return b.rows(lo, int(rm.max()) - lo + 1, M, lda)[rm - lo][:, m0:m1].double().t()
        if f["a_trans"]:
            return b.rows(k0, k1 - k0, M, lda)[:, m0:m1].double().t()
        return b.rows(m0, m1 - m0, K, lda)[:, k0:k1].double()

    def b_block(self, k0: int, k1: int) -> torch.Tensor:
        """logical B[k0:k1][0:N]"""
        f, b = self.f, self.b["B"]
        N, K, ldb = f["N"], f["K"], f["ldb"]
        if f["entry"] == "gemm_mxfp8":
            return self._dequant("B", "scale_b", f["ld_scale_b"], 0, N, k0, k1).t()
        if _k_gather(f):
            rm = self.rm_long[k0:k1]
            lo = int(rm.min())
            return b.rows(lo, int(rm.max()) - lo + 1, N, ldb)[rm - lo].double()
        if f["b_trans"]:
            return b.rows(k0, k1 - k0, N, ldb).double()
        return b.rows(0, N, K, ldb)[:, k0:k1].double().t()

    def _dequant(self, name, sname, lds, r0, r1, k0, k1):
        q = self.b[name].rows(r0, r1 - r0, self.f["K"], self.f["lda" if name == "A" else "ldb"])[:, k0:k1]
        x = q.contiguous().view(torch.float8_e4m3fn).double()
        sb = self.b[sname]
        sc = sb.t.as_strided((self.f["K"] // 128, r1 - r0), (lds, 1), sb.p + r0).to(torch.int64)
        e = torch.stack([(sc >> (8 * j)) & 0xFF for j in range(4)], -1).permute(1, 0, 2).reshape(r1 - r0, -1)   # [rows][K / 32]
        e = e[:, k0 // 32:(k1 + 31) // 32]
        return x * torch.exp2(e.double() - 127.0).repeat_interleave(32, 1)[:, k0 % 32:k0 % 32 + k1 - k0]

    def epi_inputs(self, m0: int, m1: int) -> dict:
        """fp64 epilogue operands of logical rows m0..m1"""
        f = self.f
        d = {}
        if f["bias"]:
            d["bias"] = self.b["bias"].t[self.b["bias"].p:][:f["N"]].double()
        if f["aux"]:
            if f["epilogue"] == "BF16_ADD_POS":
                a = self.b["aux"]
                pos = a.t[a.p:a.p + a.hi].double().reshape(f["seg_rows"], f["N"])
                d["aux"] = pos[torch.arange(m0, m1, device=pos.device) % f["seg_rows"]]
            else:
                d["aux"] = self.region("aux")[m0:m1].double()
        return d


# ------------------------------------------------------------------------------------------------------------ reference
def gelu(h: torch.Tensor) -> torch.Tensor:
    return 0.5 * h * (1.0 + torch.special.erf(h / math.sqrt(2.0)))


def gelu1(h: torch.Tensor) -> torch.Tensor:
    return 0.5 * (1.0 + torch.special.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


def gelu2(h: torch.Tensor) -> torch.Tensor:
    return torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi) * (2.0 - h * h)


def bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.bfloat16).double()


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """one bf16 ulp at magnitude |x| (normal range)"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def _out_bound(ref: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    return e * (1 + BF16_ROUND) + BF16_ROUND * ref.abs()


def epilogue_ref(f: dict, acc: torch.Tensor, sab: torch.Tensor, ins: dict, rows: torch.Tensor,
                 c0: Optional[torch.Tensor] = None) -> Dict[str, Tuple[torch.Tensor, torch.Tensor]]:
    """{output: (fp64 reference, per-element bound)} of logical rows `rows` given the fp64 accumulator `acc` (= A.B, alpha not applied),
    S = |alpha| |A|.|B| and the fp64 epilogue operands (bias [N], aux rows, C0 of += outputs)."""
    e = f["epilogue"]
    bias = ins.get("bias")
    aux = ins.get("aux")
    err = (KAPPA_FP8 if f["entry"] == "gemm_mxfp8" else KAPPA) * U * sab
    if bias is not None:
        err = err + U * bias.abs()
    v = acc + bias if bias is not None else acc
    out = {}
    if e == "ADD_F32":
        if aux is not None:
            err = err + U * aux.abs()
            v = v + aux
        out["C"] = (v, err)
    elif e == "ATOMIC_F32":
        ref = c0 + f["alpha"] * acc
        out["C"] = (ref, err + U * c0.abs())
    elif e == "BF16":
        out["C"] = (v, _out_bound(v, err))
    else:
        h = bf16(v)
        dh = ulp_bf16(v.abs() + err) + err                            # the kernel's intermediate: one ulp of h (+ the sum's error)
        if e == "BIAS_GELU" or e == "BIAS_GELU2":
            g = gelu(h)
            slope = torch.clamp(gelu1(h).abs() + GELU2 * dh, max=GELU1)
            eg = slope * dh + ERF_APPROX * h.abs()
            if e == "BIAS_GELU":
                out["C"] = (g, _out_bound(g, eg))
            else:
                g1 = gelu1(h)
                e1 = torch.clamp(gelu2(h).abs() + GELU3 * dh, max=GELU2) * dh + ERF_APPROX * (1 + h.abs())
                out["C"] = (g1, _out_bound(g1, e1))
                if f["C2"]:
                    out["C2"] = (g, _out_bound(g, eg))
        elif e == "MUL_GELU_GRAD":
            ref = h * aux
            out["C"] = (ref, _out_bound(ref, aux.abs() * dh + U * ref.abs()))
        elif e == "MUL_GELU_GRAD_Z":
            gz = gelu1(aux)
            ref = h * gz
            out["C"] = (ref, _out_bound(ref, gz.abs() * dh + ERF_APPROX * (1 + aux.abs()) * h.abs() + U * ref.abs()))
        elif e == "CONV_GELU":
            valid = ((rows % f["seg_rows"]) < f["seg_valid"]).double()[:, None] if f["seg_rows"] > 0 else 1.0
            g = gelu(h)
            eg = torch.clamp(gelu1(h).abs() + GELU2 * dh, max=GELU1) * dh + ERF_APPROX * h.abs()
            out["C"] = (v * valid, _out_bound(v, err) * valid)
            out["C2"] = (g * valid, _out_bound(g, eg) * valid)
        elif e == "BF16_ADD_POS":
            y = h + aux
            ey = dh + U * (y.abs() + aux.abs())
            out["C"] = (y, _out_bound(y, ey))
            if f["C2"]:
                out["C2"] = (y, ey)
        else:
            raise ValueError(f"no reference for epilogue {e}")
    if not f["C"]:
        out.pop("C", None)
    return out


def _blocks(f: dict, budget: int = 1 << 27) -> Tuple[int, int]:
    """rows per block and K per chunk so that no fp64 temporary exceeds budget elements (1 GiB)"""
    kc = f["K"] if f["K"] <= 16384 else 16384
    rb = max(16, min(f["M"], budget // max(kc, f["N"])))
    return rb, kc


def accumulate(ops_: Operands, m0: int, m1: int, k_lo: int = 0, k_hi: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp64 A.B and |A|.|B| over logical rows m0..m1 and k in [k_lo, k_hi)"""
    f = ops_.f
    k_hi = f["K"] if k_hi is None else k_hi
    _, kc = _blocks(f)
    acc = sab = None
    for k0 in range(k_lo, k_hi, kc):
        k1 = min(k_hi, k0 + kc)
        a, b = ops_.a_block(m0, m1, k0, k1), ops_.b_block(k0, k1)
        p, q = a @ b, a.abs() @ b.abs()
        acc, sab = (p, q) if acc is None else (acc + p, sab + q)
    return acc, sab * abs(f["alpha"])


class Expected:
    """fp64 reference and bound of every output of one call, over the whole output region ([M][N] in logical rows)."""

    def __init__(self, ops_: Operands, c0: Optional[Dict[str, torch.Tensor]] = None):
        f = ops_.f
        self.f = f
        self.ref: Dict[str, torch.Tensor] = {}
        self.bound: Dict[str, torch.Tensor] = {}
        rb, _ = _blocks(f)
        c0_full = None
        if f["epilogue"] == "ATOMIC_F32":
            c0_full = ops_.region("C", c0["C"]).double()
        for m0 in range(0, f["M"], rb):
            m1 = min(f["M"], m0 + rb)
            acc, sab = accumulate(ops_, m0, m1)
            rows = torch.arange(m0, m1, device=acc.device)
            outs = epilogue_ref(f, acc, sab, ops_.epi_inputs(m0, m1), rows, None if c0_full is None else c0_full[m0:m1])
            for n, (r, b) in outs.items():
                if n not in self.ref:
                    self.ref[n] = torch.empty(f["M"], f["N"], dtype=torch.float64, device=acc.device)
                    self.bound[n] = torch.empty_like(self.ref[n])
                self.ref[n][m0:m1] = r
                self.bound[n][m0:m1] = b
            del acc, sab


def reference(ops_: Operands, snapshot: Dict[str, torch.Tensor]) -> Expected:
    return Expected(ops_, snapshot)


# ------------------------------------------------------------------------------------------------------------ checks
def check(ops_: Operands, exp: Expected, snapshot: Dict[str, torch.Tensor], outs: Optional[Dict[str, torch.Tensor]] = None,
          quantize: Optional[Callable] = None, q_source: Optional[torch.Tensor] = None) -> Tuple[List[str], float]:
    """Failures (empty: the launch passed) and the largest |got - ref| / bound.  outs: {output: flat allocation} to check instead of
    the live buffers (a mutated copy); quantize(bf16 [M][N]) -> (q bytes [M][N], scale dwords [N/128][M]): q_out / q_scales must be
    exactly that of the call's own gelu(h) output (C2, or C), or of q_source when the call wrote q_out alone."""
    f = exp.f
    outs = {n: ops_.b[n].t for n in snapshot} if outs is None else outs
    fails, worst = [], 0.0
    for n, ref in exp.ref.items():
        got = ops_.region(n, outs[n]).double()
        bound = exp.bound[n]
        d = (got - ref).abs()
        finite = torch.isfinite(got)
        bad = ~finite | (d > bound)
        ratio = torch.where(bound > 0, d / bound, torch.where(d > 0, torch.full_like(d, float("inf")), torch.zeros_like(d)))
        ratio = torch.where(finite, ratio, torch.full_like(ratio, float("inf")))
        r = float(ratio.max())
        worst = max(worst, r)
        nb = int(bad.sum())
        if nb:
            i = int(torch.argmax(ratio.reshape(-1)))
            m, c = divmod(i, f["N"])
            fails.append(f"{n}: {nb} of {got.numel()} elements outside the bound (worst at row {m} col {c}: got {float(got[m, c]):.6g} "
                         f"ref {float(ref[m, c]):.6g} bound {float(bound[m, c]):.3g})")
    for n, snap in snapshot.items():
        t = outs[n].clone()
        if n in exp.ref:
            ops_.set_region(n, ops_.region(n, snap), t)
        elif n == "colsum":
            t[ops_.b[n].p:ops_.b[n].p + f["N"]] = snap[ops_.b[n].p:ops_.b[n].p + f["N"]]
        elif n == "q_out":
            ops_.b[n].rows(0, f["M"], f["N"], f["ldc"], t).copy_(ops_.b[n].rows(0, f["M"], f["N"], f["ldc"], snap))
        elif n == "q_scales":
            qs = ops_.b[n]
            qs.rows(0, f["N"] // 128, f["M"], f["ld_q_scale"], t).copy_(qs.rows(0, f["N"] // 128, f["M"], f["ld_q_scale"], snap))
        changed = _ibits(t) != _ibits(snap)
        if bool(changed.any()):
            idx = torch.nonzero(changed).reshape(-1)
            rel = [int(i) - ops_.b[n].p for i in idx[:4]]
            fails.append(f"{n}: {idx.numel()} elements outside the output region changed (offsets from the pointer {rel} ...)")
    if f["colsum"]:
        cs = ops_.b["colsum"]
        c0 = snapshot["colsum"][cs.p:cs.p + f["N"]].double()
        inc = outs["colsum"][cs.p:cs.p + f["N"]].double() - c0
        C = ops_.region("C", outs["C"]).double()
        own = C.sum(0)
        tol_own = f["M"] * U * C.abs().sum(0) + 2 * U * (c0.abs() + inc.abs())
        d_own = (inc - own).abs()
        tol_ref = exp.bound["C"].sum(0) + tol_own
        d_ref = (inc - exp.ref["C"].sum(0)).abs()
        worst = max(worst, float((d_own / tol_own).max()), float((d_ref / tol_ref).max()))
        if not bool(torch.isfinite(inc).all()) or bool((d_own > tol_own).any()) or bool((d_ref > tol_ref).any()):
            fails.append(f"colsum: increment off the column sums of C by {float(d_own.max()):.3g} (tol {float(tol_own.min()):.3g}) / of the "
                         f"reference by {float(d_ref.max()):.3g}")
    if f.get("q_out") and quantize is not None:
        src = "C2" if f["epilogue"] == "BIAS_GELU2" else "C"
        if src in outs or q_source is not None:
            q_want, s_want = quantize(ops_.region(src, outs[src]) if q_source is None else q_source)
            q_got = ops_.b["q_out"].rows(0, f["M"], f["N"], f["ldc"], outs["q_out"])
            qs = ops_.b["q_scales"]
            s_got = qs.rows(0, f["N"] // 128, f["M"], f["ld_q_scale"], outs["q_scales"])
            if not torch.equal(q_got, q_want) or not torch.equal(s_got, s_want):
                fails.append(f"q_out / q_scales: {int((q_got != q_want).sum())} bytes and {int((s_got != s_want).sum())} scale dwords differ "
                             f"from quantize({src})")
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ mutations
def _primary(exp: Expected) -> str:
    return "C" if "C" in exp.ref else "C2"


def _behind_intermediate(f: dict, name: str) -> bool:
    e = f["epilogue"]
    return e in ("BIAS_GELU", "BIAS_GELU2", "MUL_GELU_GRAD", "MUL_GELU_GRAD_Z", "BF16_ADD_POS") or (e == "CONV_GELU" and name == "C2")


def _median_element(ref: torch.Tensor) -> Tuple[int, int]:
    a = ref.abs().reshape(-1)
    step = max(1, a.numel() // (1 << 20))
    s = a[::step]
    nz = s[s > 0]
    med = float(nz.median()) if nz.numel() else 0.0
    i = int(torch.argmin((a - med).abs()))
    return divmod(i, ref.shape[1])


def mutate_ulps(ops_: Operands, exp: Expected, outs: Dict[str, torch.Tensor], name: str) -> Dict[str, torch.Tensor]:
    """One element of median |ref| moved away from the reference: 2 bf16 ulps, 4 behind a bf16 intermediate, 1e-3 relative for f32."""
    f = exp.f
    out = {n: t.clone() for n, t in outs.items()}
    m, c = _median_element(exp.ref[name])
    reg = ops_.region(name, out[name])
    got = reg[m, c:c + 1].clone()
    ref = float(exp.ref[name][m, c])
    away = 1.0 if float(got.double()) >= ref else -1.0
    if got.dtype == torch.bfloat16 and not (f["epilogue"] == "BF16_ADD_POS" and name == "C2"):
        steps = 4 if _behind_intermediate(f, name) else 2
        bits = got.view(torch.int16).int()
        sign = -1 if float(got.double()) < 0 else 1
        nb = bits + (steps if away * sign > 0 else -steps)
        got = nb.to(torch.int16).view(torch.bfloat16)
    elif _behind_intermediate(f, name):
        got = got + away * 4 * float(ulp_bf16(torch.tensor([ref], dtype=torch.float64)))
    else:
        got = got + away * 1e-3 * abs(float(got))
    reg = reg.clone()
    reg[m, c] = got[0]
    ops_.set_region(name, reg, out[name])
    return out


def mutate_row(ops_: Operands, exp: Expected, outs: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """One logical row replaced by its neighbour in every output."""
    f = exp.f
    out = {n: t.clone() for n, t in outs.items()}
    m = f["M"] // 2
    if f["seg_rows"] > 0 and f["epilogue"] == "CONV_GELU":
        m = (m // f["seg_rows"]) * f["seg_rows"]                      # a valid row with a valid neighbour
    m = min(m, f["M"] - 2)
    for n in exp.ref:
        reg = ops_.region(n, out[n]).clone()
        reg[m] = reg[m + 1]
        ops_.set_region(n, reg, out[n])
    return out


def _recompute(ops_: Operands, exp: Expected, outs, m0, m1, n0, n1, dacc: torch.Tensor, drop_bias_col: Optional[int] = None):
    """Outputs of the block rows m0..m1 x cols n0..n1 recomputed by the reference's epilogue from acc + dacc (and the bias of one column
    dropped), rounded to each output's type: what a kernel with that accumulator would store."""
    f = exp.f
    out = {n: t.clone() for n, t in outs.items()}
    acc, sab = accumulate(ops_, m0, m1)
    acc = acc.clone()
    acc[:, n0:n1] += dacc
    ins = ops_.epi_inputs(m0, m1)
    c0 = None
    if f["epilogue"] == "ATOMIC_F32":
        c0 = (exp.ref["C"][m0:m1] - f["alpha"] * accumulate(ops_, m0, m1)[0])
    if drop_bias_col is not None:
        ins = dict(ins)
        ins["bias"] = ins["bias"].clone()
        ins["bias"][drop_bias_col] = 0.0
    new = epilogue_ref(f, acc, sab, ins, torch.arange(m0, m1, device=acc.device), c0)
    for n, (r, _) in new.items():
        reg = ops_.region(n, out[n]).clone()
        reg[m0:m1, n0:n1] = r[:, n0:n1].to(reg.dtype)
        ops_.set_region(n, reg, out[n])
    return out


def mutate_kslice(ops_: Operands, exp: Expected, outs) -> Dict[str, torch.Tensor]:
    """One 32-wide k-slice's contribution removed from one 16 x 16 block (the fp64 partial product)."""
    f = exp.f
    m0 = min(f["M"] - 16, (f["M"] // 3) // 16 * 16) if f["M"] >= 16 else 0
    n0 = min(f["N"] - 16, (f["N"] // 2) // 16 * 16) if f["N"] >= 16 else 0
    m1, n1 = min(f["M"], m0 + 16), min(f["N"], n0 + 16)
    k0 = (f["K"] // 2) // 32 * 32
    k1 = min(f["K"], k0 + 32)
    part = accumulate(ops_, m0, m1, k0, k1)[0][:, n0:n1]
    return _recompute(ops_, exp, outs, m0, m1, n0, n1, -part)


def _kps(K: int, split: int) -> int:
    """K per split as csrc/gemm.hip cuts it (64-deep multiples)"""
    return ((K + split - 1) // split + 63) // 64 * 64


def mutate_split(ops_: Operands, exp: Expected, outs, split: int, double: bool) -> Dict[str, torch.Tensor]:
    """One K split's share of one 256 x 128 tile dropped (or counted twice)."""
    f = exp.f
    kps = _kps(f["K"], split)
    s = min(-(-f["K"] // kps) - 1, 1)
    k0, k1 = s * kps, min(f["K"], (s + 1) * kps)
    m0, n0 = 0, (f["N"] // 2) // 128 * 128
    m1, n1 = min(f["M"], 256), min(f["N"], n0 + 128)
    part = accumulate(ops_, m0, m1, k0, k1)[0][:, n0:n1] * f["alpha"]
    return _recompute(ops_, exp, outs, m0, m1, n0, n1, part if double else -part)


def mutate_bias(ops_: Operands, exp: Expected, outs) -> Dict[str, torch.Tensor]:
    """The bias of one column dropped."""
    f = exp.f
    n, m1 = f["N"] // 3, min(f["M"], 2048)
    return _recompute(ops_, exp, outs, 0, m1, n, n + 1, torch.zeros(m1, 1, dtype=torch.float64, device=exp.ref[_primary(exp)].device),
                      drop_bias_col=n)


def mutations(ops_: Operands, exp: Expected, outs, split: int = 1):
    """(name, mutated outputs) for every mutation that applies to this call."""
    f = exp.f
    if not exp.ref:                      # q_out alone (fp8 teacher linear1): checked bit for bit against its bf16 twin instead
        return
    for n in exp.ref:
        yield f"{n} moved off by ulps", mutate_ulps(ops_, exp, outs, n)
    if f["M"] >= 2:
        yield "row replaced by its neighbour", mutate_row(ops_, exp, outs)
    if f["K"] > 32:
        yield "k-slice dropped from a 16x16 block", mutate_kslice(ops_, exp, outs)
    if split > 1 and f["K"] > _kps(f["K"], split):
        yield "K split's share dropped", mutate_split(ops_, exp, outs, split, False)
        yield "K split's share doubled", mutate_split(ops_, exp, outs, split, True)
    if f["bias"]:
        yield "bias of one column dropped", mutate_bias(ops_, exp, outs)
