"""fp64 reference, per-element error bound and region checks for single wj_attn_fwd / wj_attn_bwd calls (test infrastructure; used by
tests/test_attention_reference_cpu.py and tests/test_attention_census_gpu.py; the buffer and bit helpers are tests/gemm_reference.py's).

A call is a plain dict (`fields`): B, T, H, hd, form = "none" | "mask" | "ragged", mask_group, the key mask (bool [ceil(B / mask_group)][T],
True = key NOT attended) or the seq_off list (int32 [B + 1]), lse wanted, dbias, defer_fold.  `Operands` allocates qkv / dout and every
output (out, lse, dqkv, dbias, dbias_ws) inside a larger allocation with guard bands on both sides, fills the inputs with seeded bf16
data of a named regime and the outputs with NaN (dbias, which is accumulated into, with known finite values).  `reference_fwd` /
`reference_bwd` compute the fp64 result from the bf16 inputs together with a bound per element (no norm anywhere); `check` holds what
a launch wrote against them; `mutations` edits a copy of a passing output the way a subtly broken kernel would.

Data regimes (REGIMES):
  flat     unit normal q, k, v: scaled scores of standard deviation ~1, a nearly flat softmax
  peaked   q, k scaled by sqrt(8): scaled scores of standard deviation ~8, most rows close to one-hot
  offset   a common +-OFFSET vector added to k and, with the sign of the head's half, to q: every score of a row sits near
           +OFFSET^2 sqrt(hd) (heads < H/2) or -OFFSET^2 sqrt(hd) (the others) -- the max subtraction and the lse magnitude
  planted  flat, plus in every sequence (query, key) pairs of magnitude PLANT aligned or anti-aligned in all hd dimensions: query 0 with
           the last valid key (+), query min(15, L-1) with key min(16, L-1) (-), the last valid row with the first masked key, or key 0
           where nothing is masked (+)
  extreme  the overflow probe: in even sequences the last valid row is aligned with the first masked key, in odd sequences query 0 is
           anti-aligned with EVERY key, at the smallest magnitude a (multiples of 1/4, exact in bf16; all hd elements of the planted
           rows are +-a) at which fp64 says the masked key's scaled score exceeds its row's lse by more than 90 (key-mask form) and the
           odd sequences' row 0 has lse < -90.  `Operands.extreme_scale` is that a.

Rounding points of the kernels (wavjepa_amd/csrc/attention.hip) and the terms they give (u = 2^-9 bf16, u32 = 2^-24 fp32):
  forward   :184 scores S = K Q^T in the MFMA's fp32 from exact bf16 products        dscore = hd u32 scale |q|.|k|
            :203 p = exp2(fma(s, scale log2 e, -max scale log2 e)) in fp32            + 4 u32 (|s scale| + |max scale| + 1)     =: e
            :209-210 sum over keys in fp32, inv = 1 / sum                            ebar = sum_k P e  (+ T u32)
            :218 P = p * inv rounded to bf16                                         u
            :221 O^T = V^T P^T accumulated in fp32 over the keys                      T u32
            :231 out rounded to bf16                                                 u |out|
            :235 lse = fma(max, scale, log(sum))                                     ebar + T u32 + 2 u32 (|max scale| + |log sum| + |lse|)
                                                                                     + 2^-22 (1 + |log sum|) for v_log_f32
    |out - ref|  <= KAPPA [ sum_k P_k (u + e_k + ebar + T u32) |v_kd| (1 + u) + u |ref| ] + 2^-133
  backward  :339/:417/:591/:672 scores as the forward; :345/:424/:599-600/:680-681 p = exp2(s scale log2 e + mask - lse log2 e) from the
            STORED fp32 lse: e_p = e + |lse given - lse ref| (never more than the forward's lse bound) + 2 u32 |lse|
            :340 dP = V dO^T in fp32: ddP = hd u32 |dO|.|v|;   :297/:548 delta = sum_d dO O in fp32 from the bf16 out the backward is
            given: ddelta = hd u32 sum |dO O|
            :346/:601 dS = p (dP - delta) (scale) and :425/:682 P rounded to bf16 by pack_tiles (:350/:430-431/:605/:687-688)      u
            :353/:434 second MFMA accumulates in fp32 over T                         T u32
            :362/:446/:620/:704 dq, dk, dv rounded to bf16                           u |ref|
    W = |dS| (u + e_p + T u32) + P scale (ddP + ddelta);   |dq - ref| <= KAPPA [ (W |K|)(1 + u) + u |ref| ] + 2^-133, dk with W^T |Q|,
    dv with (P (u + e_p + T u32))^T |dO|.
  dbias     fp32 sums of the bf16-rounded dqkv (the header's definition): in-thread chain over the wave's tiles (:362), 4 cross-lane adds
            (:375), LDS atomics of the 4 waves (:376), the fold of the B rows (wj_colsum_f32: <= 8 rows per thread, 8 row lanes, <= 32
            workgroups' atomics).  |dbias_ws - colsum_b| <= KAPPA u32 (T / 64 + 12) sum |x|;  the folded dbias adds (B / 256 + 48).
KAPPA multiplies every computed term.  It is NOT fitted to the HIP kernel: tests/test_attention_reference_cpu.py's emulation of the
arithmetic above (fp32, bf16 at the listed points) must pass at it in every regime while every mutation stays rejected; the emulation's
worst element sits at 1.0-1.75 times the KAPPA = 1 bound (out 1.0-1.6, dqkv 1.1-1.75, lse below 0.08), so 4 leaves a factor 2.3; how
much loosening blinds the mutations is pinned in that test.

Memory: the reference walks the batch in chunks of n sequences with n H T^2 <= 2^24 elements; about a dozen fp64 [n][H][T][T] tensors
are alive at once, so the peak is ~1.6 GB whatever B is (256 x 12 heads at T = 400: 8 sequences per chunk, 32 chunks).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.gemm_reference import Buf, _gen, _ibits, _nan_bits

U16 = 2.0 ** -9
U32 = 2.0 ** -24
KAPPA = 4.0            # see the module docstring and tests/test_attention_reference_cpu.py (emulation <= 1.75 at KAPPA = 1)
TINY = 2.0 ** -133     # smallest bf16 subnormal step
TINY32 = 2.0 ** -149
LOG2E = 1.4426950408889634
REGIMES = ("flat", "peaked", "offset", "planted", "extreme")
PEAK = math.sqrt(8.0)
OFFSET = 1.5
PLANT = 1.5
CHUNK_ELEMS = 1 << 24
LAST: Dict[str, float] = {}     # worst err / bound per output of the last check()


# ------------------------------------------------------------------------------------------------------------ fields
def fields(B: int, T: int, H: int, hd: int, form: str = "none", mask=None, seq_off=None, mask_group: int = 1, lse: bool = True,
           dbias: bool = True, defer_fold: bool = False) -> dict:
    assert form in ("none", "mask", "ragged")
    f = dict(B=int(B), T=int(T), H=int(H), hd=int(hd), form=form, mask_group=int(mask_group), lse=bool(lse), dbias=bool(dbias),
             defer_fold=bool(defer_fold), mask=None, seq_off=None)
    if form == "mask":
        m = np.ascontiguousarray(np.asarray(mask, dtype=bool))
        assert m.shape == ((B + mask_group - 1) // mask_group, T), m.shape
        f["mask"] = m
    if form == "ragged":
        s = np.ascontiguousarray(np.asarray(seq_off, dtype=np.int32))
        assert s.shape == (B + 1,) and s[0] == 0 and (np.diff(s) >= 0).all() and int(np.diff(s).max()) <= T, s
        f["seq_off"] = s
    return f


def signature(f: dict) -> tuple:
    return tuple((k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(f.items()))


def describe(f: dict) -> str:
    s = f"B={f['B']} T={f['T']} H={f['H']} hd={f['hd']} {f['form']}"
    if f["form"] == "mask":
        s += f" mask_group={f['mask_group']} masked={float(f['mask'].mean()):.2f}"
    if f["form"] == "ragged":
        ln = np.diff(f["seq_off"])
        s += f" rows={int(f['seq_off'][-1])} len={int(ln.min())}..{int(ln.max())}"
    return s + f" lse={int(f['lse'])} dbias={int(f['dbias'])} defer_fold={int(f['defer_fold'])}"


def n_rows(f: dict) -> int:
    return int(f["seq_off"][-1]) if f["form"] == "ragged" else f["B"] * f["T"]


class Index:
    """Per sequence: length, first row, and on the padded [B][Tm] grid which rows exist (qval), which keys are attended (kval) and the
    packed row of every grid point (row; 0 where the row does not exist)."""

    def __init__(self, f: dict, device):
        B, T = f["B"], f["T"]
        if f["form"] == "ragged":
            off = torch.as_tensor(f["seq_off"].astype(np.int64), device=device)
            self.len, self.row0 = off[1:] - off[:-1], off[:-1]
            self.Tm = max(int(self.len.max()), 1)
        else:
            self.len = torch.full((B,), T, dtype=torch.long, device=device)
            self.row0 = torch.arange(B, device=device) * T
            self.Tm = T
        t = torch.arange(self.Tm, device=device)
        self.qval = t[None, :] < self.len[:, None]
        self.kval = self.qval.clone()
        if f["form"] == "mask":
            m = torch.as_tensor(f["mask"], device=device)
            self.kval = ~m[torch.arange(B, device=device) // f["mask_group"]]
        self.row = torch.where(self.qval, self.row0[:, None] + t[None, :], torch.zeros_like(t)[None, :])


# ------------------------------------------------------------------------------------------------------------ operands
class Operands:
    """Every operand of one call (forward and backward share them), allocated with guard bands and filled."""

    def __init__(self, f: dict, device, seed: int = 0, regime: str = "flat"):
        assert regime in REGIMES
        self.f, self.device, self.regime = f, device, regime
        B, T, H, hd = f["B"], f["T"], f["H"], f["hd"]
        D, R = H * hd, n_rows(f)
        self.D, self.R = D, R
        self.ix = Index(f, device)
        bf, f32 = torch.bfloat16, torch.float32
        self.n_lse = R * H
        self.b = {"qkv": Buf(0, max(R, 1) * 3 * D, bf, 3 * D, None, device), "dout": Buf(0, max(R, 1) * D, bf, D, None, device),
                  "out": Buf(0, max(R, 1) * D, bf, D, None, device), "lse": Buf(0, max(self.n_lse, 1), f32, H, None, device),
                  "dqkv": Buf(0, max(R, 1) * 3 * D, bf, 3 * D, None, device), "dbias": Buf(0, 3 * D, f32, 3 * D, None, device),
                  "dbias_ws": Buf(0, B * 3 * D, f32, 3 * D, None, device)}
        self.key_mask = None if f["form"] != "mask" else torch.as_tensor(f["mask"]).to(torch.uint8).contiguous().to(device)
        self.seq_off = None if f["form"] != "ragged" else torch.as_tensor(f["seq_off"]).to(device)
        self.extreme_scale = None
        g = _gen(seed, device)
        base = torch.randn((R, 3, H, hd), generator=g, dtype=torch.float32, device=device)
        self.view("dout")[:] = torch.randn((R, D), generator=g, dtype=torch.float32, device=device).to(bf)
        sign = (torch.randint(0, 2, (B, H, hd), generator=g, device=device) * 2 - 1).float()
        if regime == "extreme":
            a = 1.0
            while True:
                self.view("qkv")[:] = self._shape_inputs(base, sign, regime, a).reshape(R, 3 * D).to(bf)
                if self._extreme_reached() or a >= 16.0:
                    break
                a += 0.25
            assert a < 16.0, "the extreme regime found no magnitude below 16"
            self.extreme_scale = a
        else:
            self.view("qkv")[:] = self._shape_inputs(base, sign, regime, PLANT).reshape(R, 3 * D).to(bf)
        self.reset_outputs()

    # ---- data
    def _planted_rows(self):
        """(first masked key or key 0, last valid row, last visible key) per sequence, as packed rows; valid = the sequence has a row"""
        ix = self.ix
        L = ix.len
        has = L > 0
        last = torch.clamp(L - 1, min=0)
        t = torch.arange(ix.Tm, device=self.device)[None, :]
        masked = ix.qval & ~ix.kval
        first_masked = torch.where(masked.any(1), masked.float().argmax(1), torch.zeros_like(L))
        last_vis = torch.where(ix.kval.any(1), (ix.kval * (t + 1)).amax(1) - 1, last)
        return has, last, first_masked, last_vis

    def _shape_inputs(self, base: torch.Tensor, sign: torch.Tensor, regime: str, a: float) -> torch.Tensor:
        f, ix = self.f, self.ix
        H = f["H"]
        x = base.clone()
        if regime == "peaked":
            x[:, :2] *= PEAK
        if regime == "offset":
            u = sign[0, 0]                                                       # one +-1 vector for the whole call
            hs = torch.where(torch.arange(H, device=self.device) < (H + 1) // 2, 1.0, -1.0)
            x[:, 1] += OFFSET * u
            x[:, 0] += OFFSET * u * hs[:, None]
        if regime in ("planted", "extreme") and self.R > 0:
            has, last, fm, lv = self._planted_rows()
            r0 = ix.row0
            L = ix.len
            w = sign * a
            sel = has.clone()
            if regime == "extreme":
                odd = (torch.arange(f["B"], device=self.device) % 2 == 1) & has
                for b in torch.nonzero(odd).flatten().tolist():                  # query 0 against every key of the sequence
                    rows = slice(int(r0[b]), int(r0[b] + L[b]))
                    x[rows, 1] = -w[b] + 0.25 * x[rows, 1]
                    x[int(r0[b]), 0] = w[b]
                sel = has & ~odd
            else:
                b_ = torch.nonzero(has).flatten()
                x[(r0 + 0)[b_], 0] = w[b_]
                x[(r0 + lv)[b_], 1] = w[b_]
                q2, k2 = torch.clamp(L - 1, max=15, min=0), torch.clamp(L - 1, max=16, min=0)
                x[(r0 + q2)[b_], 0] = torch.roll(w, 1, -1)[b_]
                x[(r0 + k2)[b_], 1] = -torch.roll(w, 1, -1)[b_]
            b_ = torch.nonzero(sel).flatten()
            x[(r0 + last)[b_], 0] = torch.roll(w, 2, -1)[b_]
            x[(r0 + fm)[b_], 1] = torch.roll(w, 2, -1)[b_]
        return x

    def _extreme_reached(self) -> bool:
        f, ix = self.f, self.ix
        has, last, fm, lv = self._planted_rows()
        qkv = self.view("qkv").double().reshape(self.R, 3, f["H"], f["hd"])
        scale = 1.0 / math.sqrt(f["hd"])
        ok_mask, ok_low = f["form"] != "mask", False
        for b in range(f["B"]):
            if not bool(has[b]):
                continue
            r0, L = int(ix.row0[b]), int(ix.len[b])
            k = qkv[r0:r0 + L, 1]
            qrow = 0 if b % 2 else int(last[b])
            s = torch.einsum("hd,thd->ht", qkv[r0 + qrow, 0], k) * scale
            lse = torch.logsumexp(s.masked_fill(~ix.kval[b, :L][None, :], float("-inf")), -1)
            if b % 2:
                ok_low |= bool((lse < -90).any()) and L % 16 != 0
            elif f["form"] == "mask" and not bool(ix.kval[b, int(fm[b])]):
                ok_mask |= bool((s[:, int(fm[b])] - lse > 90).any())
        return ok_mask and ok_low

    # ---- views and resets
    def view(self, name: str, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """the region of an operand as its logical matrix (qkv / dqkv [R][3D], out / dout [R][D], dbias [3D], dbias_ws [B][3D],
        lse flat)"""
        b = self.b[name]
        t = b.t if t is None else t
        D, R = self.D, self.R
        if name in ("qkv", "dqkv"):
            return b.rows(0, R, 3 * D, 3 * D, t)
        if name in ("out", "dout"):
            return b.rows(0, R, D, D, t)
        if name == "dbias_ws":
            return b.rows(0, self.f["B"], 3 * D, 3 * D, t)
        if name == "dbias":
            return t[b.p:b.p + 3 * D]
        return t[b.p:b.p + self.n_lse]

    def lse_rows(self, t: Optional[torch.Tensor] = None) -> torch.Tensor:
        """lse as [R][H] whatever the layout (dense: [B][H][T] in memory)"""
        f = self.f
        v = self.view("lse", t)
        if f["form"] == "ragged":
            return v.reshape(self.R, f["H"])
        return v.reshape(f["B"], f["H"], f["T"]).permute(0, 2, 1).reshape(self.R, f["H"])

    def set_lse_rows(self, rows: torch.Tensor, t: torch.Tensor) -> None:
        f = self.f
        v = self.view("lse", t)
        if f["form"] == "ragged":
            v.copy_(rows.reshape(-1))
        else:
            v.copy_(rows.reshape(f["B"], f["T"], f["H"]).permute(0, 2, 1).reshape(-1))

    def region_len(self, name: str) -> int:
        D, R = self.D, self.R
        return {"out": R * D, "dqkv": R * 3 * D, "lse": self.n_lse, "dbias": 3 * D, "dbias_ws": self.f["B"] * 3 * D}[name]

    def dbias_seed(self) -> torch.Tensor:
        return 1.0 + 0.125 * (torch.arange(3 * self.D, device=self.device) % 7).float()

    def output_names(self, phase: str) -> List[str]:
        if phase == "fwd":
            return ["out"] + (["lse"] if self.f["lse"] else [])
        return ["dqkv"] + (["dbias", "dbias_ws"] if self.f["dbias"] else [])

    def reset_outputs(self, phase: Optional[str] = None) -> None:
        for name in (["out", "lse", "dqkv", "dbias", "dbias_ws"] if phase is None else
                     {"fwd": ["out", "lse"], "bwd": ["dqkv", "dbias", "dbias_ws"]}[phase]):
            b = self.b[name]
            _ibits(b.t).fill_(_nan_bits(b.dt))
        if phase in (None, "bwd"):
            self.view("dbias").copy_(self.dbias_seed())

    def snapshot(self, phase: str) -> Dict[str, torch.Tensor]:
        return {n: self.b[n].t.clone() for n in (["out", "lse"] if phase == "fwd" else ["dqkv", "dbias", "dbias_ws"])}

    def fwd_kwargs(self) -> dict:
        f, b = self.f, self.b
        return dict(qkv=b["qkv"].ptr, out=b["out"].ptr, B=f["B"], T=f["T"], H=f["H"], hd=f["hd"], key_mask=self.key_mask,
                    lse=b["lse"].ptr if f["lse"] else None, mask_group=f["mask_group"], seq_off=self.seq_off)

    def bwd_kwargs(self, defer_fold: Optional[bool] = None) -> dict:
        f, b = self.f, self.b
        return dict(qkv=b["qkv"].ptr, out=b["out"].ptr, dout=b["dout"].ptr, lse=b["lse"].ptr, dqkv=b["dqkv"].ptr, B=f["B"], T=f["T"],
                    H=f["H"], hd=f["hd"], key_mask=self.key_mask, mask_group=f["mask_group"], seq_off=self.seq_off,
                    dbias=b["dbias"].ptr if f["dbias"] else None, dbias_ws=b["dbias_ws"].ptr if f["dbias"] else None,
                    defer_fold=f["defer_fold"] if defer_fold is None else defer_fold)


# ------------------------------------------------------------------------------------------------------------ reference
def core(q, k, v, kval, qval, scale: float, hd: int, dO=None, O=None, dlse=None, keep: bool = False) -> dict:
    """fp64 attention of [n][H][T][hd] operands with attended keys kval [n][T] and existing rows qval [n][T]: out, lse and their bound
    terms; with dO / O (the bf16 out the backward is given) / dlse (|lse given - lse ref| per row) also dq, dk, dv and theirs."""
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
    del E, S
    lsum = torch.log(torch.where(ssum > 0, ssum, torch.ones_like(ssum)))
    lse = torch.where(dead, torch.full_like(m0, float("inf")), m0 + lsum)
    e = e + 4 * U32 * m0.abs()
    ebar = (P * e).sum(-1, keepdim=True)
    r = {"out": P @ v, "lse": lse[..., 0], "dead": dead[..., 0]}
    r["out_e"] = (P * (U16 + e + ebar + T * U32)) @ av
    r["lse_e"] = (ebar + T * U32 + 2 * U32 * (m0.abs() + lsum.abs() + torch.where(dead, torch.zeros_like(lse), lse).abs())
                  + 2.0 ** -22 * (1.0 + lsum.abs()))[..., 0]
    if dO is None:
        return r
    adO = dO.abs()
    dP = dO @ v.transpose(-1, -2)
    ddP = hd * U32 * (adO @ av.transpose(-1, -2))
    delta = (dO * O).sum(-1, keepdim=True)
    ddelta = hd * U32 * (adO * O.abs()).sum(-1, keepdim=True)
    dS = P * (dP - delta) * scale
    ep = e + dlse[..., None] + 2 * U32 * torch.where(dead, torch.zeros_like(lse), lse).abs() + T * U32 + U16
    W = dS.abs() * ep + P * scale * (ddP + ddelta)
    del dP, ddP, e
    r["dq"], r["dq_e"] = dS @ k, W @ ak
    r["dk"], r["dk_e"] = dS.transpose(-1, -2) @ q, W.transpose(-1, -2) @ aq
    r["dv"], r["dv_e"] = P.transpose(-1, -2) @ dO, (P * ep).transpose(-1, -2) @ adO
    if keep:
        r["dS"], r["P"] = dS, P
    return r


def out_bound(ref: torch.Tensor, e: torch.Tensor, kappa: float) -> torch.Tensor:
    return kappa * (e * (1.0 + U16) + U16 * ref.abs()) + TINY


class Expected:
    def __init__(self):
        self.ref: Dict[str, torch.Tensor] = {}
        self.bound: Dict[str, torch.Tensor] = {}


def _chunks(f: dict, Tm: int):
    n = max(1, CHUNK_ELEMS // max(1, f["H"] * Tm * Tm))
    return [(b0, min(f["B"], b0 + n)) for b0 in range(0, f["B"], n)]


def _gather(o: Operands, name: str, b0: int, b1: int, part: Optional[int] = None, t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[n][H][Tm][hd] fp64 of the rows of sequences b0..b1 (q / k / v: part 0 / 1 / 2 of qkv)"""
    f, ix = o.f, o.ix
    H, hd = f["H"], f["hd"]
    rows = ix.row[b0:b1].reshape(-1)
    x = o.view(name, t)[rows]
    x = x.reshape(b1 - b0, ix.Tm, -1, H, hd)[:, :, 0 if part is None else part]
    return x.permute(0, 2, 1, 3).double()


def _scatter(o: Operands, dst: torch.Tensor, val: torch.Tensor, b0: int, b1: int) -> None:
    """val [n][H][Tm][w] -> dst [R][H * w] on the existing rows"""
    ix = o.ix
    qv = ix.qval[b0:b1].reshape(-1)
    v = val.permute(0, 2, 1, 3).reshape(qv.numel(), -1)
    dst[ix.row[b0:b1].reshape(-1)[qv]] = v[qv]


def reference_fwd(o: Operands, kappa: float = KAPPA) -> Expected:
    f, ix, dev = o.f, o.ix, o.device
    H, hd, D, R = f["H"], f["hd"], o.D, o.R
    ex = Expected()
    out, oe = torch.zeros(R, D, dtype=torch.float64, device=dev), torch.zeros(R, D, dtype=torch.float64, device=dev)
    lse, le = torch.zeros(R, H, dtype=torch.float64, device=dev), torch.zeros(R, H, dtype=torch.float64, device=dev)
    dead = torch.zeros(R, H, dtype=torch.bool, device=dev)
    for b0, b1 in _chunks(f, ix.Tm):
        r = core(_gather(o, "qkv", b0, b1, 0), _gather(o, "qkv", b0, b1, 1), _gather(o, "qkv", b0, b1, 2), ix.kval[b0:b1], ix.qval[b0:b1],
                 1.0 / math.sqrt(hd), hd)
        _scatter(o, out, r["out"], b0, b1)
        _scatter(o, oe, r["out_e"], b0, b1)
        for dst, key in ((lse, "lse"), (le, "lse_e"), (dead, "dead")):
            _scatter(o, dst, r[key][..., None], b0, b1)
    ex.ref["out"], ex.bound["out"] = out, torch.where(dead.repeat_interleave(hd, 1), torch.zeros_like(oe), out_bound(out, oe, kappa))
    ex.ref["lse"], ex.bound["lse"] = lse, kappa * le
    ex.dead = dead
    return ex


def reference_bwd(o: Operands, fwd: Expected, out_t: Optional[torch.Tensor] = None, lse_t: Optional[torch.Tensor] = None,
                  kappa: float = KAPPA) -> Expected:
    """out_t / lse_t: the allocations holding the bf16 out and the fp32 lse the backward is given (default: the operands' own)"""
    f, ix, dev = o.f, o.ix, o.device
    H, hd, D, R = f["H"], f["hd"], o.D, o.R
    ex = Expected()
    ref = torch.zeros(R, 3 * D, dtype=torch.float64, device=dev)
    err = torch.zeros(R, 3 * D, dtype=torch.float64, device=dev)
    given = o.lse_rows(lse_t).double()
    d = (given - fwd.ref["lse"]).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    dl = torch.minimum(d, fwd.bound["lse"])
    for b0, b1 in _chunks(f, ix.Tm):
        n = b1 - b0
        dlc = dl[ix.row[b0:b1].reshape(-1)].reshape(n, ix.Tm, H).permute(0, 2, 1)
        r = core(_gather(o, "qkv", b0, b1, 0), _gather(o, "qkv", b0, b1, 1), _gather(o, "qkv", b0, b1, 2), ix.kval[b0:b1], ix.qval[b0:b1],
                 1.0 / math.sqrt(hd), hd, dO=_gather(o, "dout", b0, b1), O=_gather(o, "out", b0, b1, t=out_t), dlse=dlc)
        for j, key in enumerate(("dq", "dk", "dv")):
            _scatter(o, ref[:, j * D:(j + 1) * D], r[key], b0, b1)
            _scatter(o, err[:, j * D:(j + 1) * D], r[key + "_e"], b0, b1)
    bound = out_bound(ref, err, kappa)
    mk = torch.zeros(R, dtype=torch.bool, device=dev)                       # rows of masked keys: dk, dv exactly 0
    mk[ix.row[ix.qval & ~ix.kval]] = True
    bound[:, D:] = torch.where(mk[:, None], torch.zeros_like(bound[:, D:]), bound[:, D:])
    bound[:, :D] = torch.where(fwd.dead.repeat_interleave(hd, 1), torch.zeros_like(bound[:, :D]), bound[:, :D])
    ex.ref["dqkv"], ex.bound["dqkv"] = ref, bound
    ex.masked_key_rows = mk
    return ex


# ------------------------------------------------------------------------------------------------------------ check
def _seq_of_row(o: Operands) -> torch.Tensor:
    ix = o.ix
    s = torch.zeros(max(o.R, 1), dtype=torch.long, device=o.device)
    b = torch.arange(o.f["B"], device=o.device)[:, None].expand_as(ix.row)
    s[ix.row[ix.qval]] = b[ix.qval]
    return s


def check(o: Operands, ex: Expected, snap: Dict[str, torch.Tensor], phase: str, outs: Optional[Dict[str, torch.Tensor]] = None,
          kappa: float = KAPPA, folded: Optional[bool] = None, slack: float = 0.0) -> Tuple[List[str], float]:
    """What a launch left in the output allocations (or `outs`) against the reference: (failures, worst err / bound).
    folded: whether the launch folded dbias (default: not f['defer_fold']).  slack: a deliberately WRONG additive term, slack times the
    largest |ref| of the tensor, for the test that shows what a norm-wide floor would hide."""
    f = o.f
    D, R, B, T = o.D, o.R, f["B"], f["T"]
    fails, worst = [], 0.0
    LAST.clear()
    folded = (not f["defer_fold"]) if folded is None else folded
    scale_k = kappa / KAPPA

    def tens(name):
        return o.b[name].t if outs is None or name not in outs else outs[name]

    def outside(name):
        b, t = o.b[name], tens(name)
        n = o.region_len(name)
        a, s = _ibits(t), _ibits(snap[name])
        bad = int((a[:b.p] != s[:b.p]).sum()) + int((a[b.p + n:] != s[b.p + n:]).sum())
        if bad:
            fails.append(f"{name}: {bad} elements outside the region changed")

    def inside(name, got, ref, bound, exact=None):
        nonlocal worst
        got = got.double()
        if slack:
            fin = ref[torch.isfinite(ref)]
            bound = bound + slack * (float(fin.abs().max()) if fin.numel() else 0.0)
        special = ~torch.isfinite(ref)
        nf = ~torch.isfinite(got) & ~special
        if bool(nf.any()):
            fails.append(f"{name}: {int(nf.sum())} elements not finite (first at {torch.nonzero(nf)[0].tolist()})")
        if bool(special.any()) and not bool((got[special] == ref[special]).all()):
            fails.append(f"{name}: {int((got[special] != ref[special]).sum())} special values (fully masked rows) not as promised")
        ok = ~special & ~nf
        err = torch.where(ok, (got - ref).abs(), torch.zeros_like(ref))
        ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
        w = float(ratio.max()) if ratio.numel() else 0.0
        LAST[name] = w
        worst = max(worst, w)
        bad = ok & (err > bound)
        if bool(bad.any()):
            i = torch.nonzero(bad)[0].tolist()
            fails.append(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the bound (worst err/bound {w:.3g}; first at {i}: "
                         f"got {float(got[tuple(i)]):.6g}, ref {float(ref[tuple(i)]):.6g}, bound {float(bound[tuple(i)]):.3g})")

    if phase == "fwd":
        outside("out")
        inside("out", o.view("out", tens("out")), ex.ref["out"], ex.bound["out"] * scale_k)
        outside("lse")
        if f["lse"]:
            inside("lse", o.lse_rows(tens("lse")), ex.ref["lse"], ex.bound["lse"] * scale_k)
        else:
            b = o.b["lse"]
            if not torch.equal(_ibits(tens("lse")), _ibits(snap["lse"])):
                fails.append("lse: written although not asked for")
        return fails, worst
    outside("dqkv")
    got = o.view("dqkv", tens("dqkv"))
    inside("dqkv", got, ex.ref["dqkv"], ex.bound["dqkv"] * scale_k)
    mk = ex.masked_key_rows
    if bool(mk.any()) and float(got[mk][:, D:].float().abs().max()) != 0.0:
        fails.append("dqkv: dk / dv rows of masked keys not exactly 0")
    for name in ("dbias", "dbias_ws"):
        outside(name)
    if not f["dbias"]:
        for name in ("dbias", "dbias_ws"):
            if not torch.equal(_ibits(tens(name)), _ibits(snap[name])):
                fails.append(f"{name}: written although dbias was not asked for")
        return fails, worst
    x = got.double()
    x = torch.where(torch.isfinite(x), x, torch.zeros_like(x))               # (a NaN in dqkv is reported above, once)
    seq = _seq_of_row(o)
    part = torch.zeros(B, 3 * D, dtype=torch.float64, device=o.device).index_add_(0, seq[:R], x)
    apart = torch.zeros(B, 3 * D, dtype=torch.float64, device=o.device).index_add_(0, seq[:R], x.abs())
    ws = o.view("dbias_ws", tens("dbias_ws"))
    inside("dbias_ws", ws, part, kappa * U32 * (T / 64 + 12) * apart + TINY32)
    empty = o.ix.len == 0
    if bool(empty.any()) and float(ws[empty].abs().max()) != 0.0:
        fails.append("dbias_ws: rows of empty sequences not 0")
    seed = o.dbias_seed().double()
    db = o.view("dbias", tens("dbias"))
    if not folded:
        if not torch.equal(_ibits(tens("dbias")), _ibits(snap["dbias"])):
            fails.append("dbias: changed although the fold was deferred")
        return fails, worst
    bsum = kappa * U32 * (T / 64 + 12 + B / 256 + 48) * apart.sum(0) + 2 * U32 * seed.abs() + TINY32
    inside("dbias", db, seed + part.sum(0), bsum)
    rb = ex.bound["dqkv"] * scale_k
    inside("dbias_vs_ref", db, seed + ex.ref["dqkv"].sum(0), bsum + torch.where(torch.isfinite(rb), rb, torch.zeros_like(rb)).sum(0))
    return fails, worst


# ------------------------------------------------------------------------------------------------------------ mutations
def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16)


class _Head:
    """one (b, h) of a call in fp64, with the bf16 out it was given"""

    def __init__(self, o: Operands, b: int, h: int, out_t: torch.Tensor):
        f, ix = o.f, o.ix
        hd = f["hd"]
        self.o, self.b, self.h = o, b, h
        self.L, self.r0 = int(ix.len[b]), int(ix.row0[b])
        rows = slice(self.r0, self.r0 + self.L)
        c = slice(h * hd, (h + 1) * hd)
        qkv = o.view("qkv")[rows].double().reshape(self.L, 3, f["H"], hd)[:, :, h]
        self.q, self.k, self.v = (qkv[:, j][None, None] for j in range(3))
        self.dO = o.view("dout")[rows, c].double()[None, None]
        self.O = o.view("out", out_t)[rows, c].double()[None, None]
        self.kval = ix.kval[b, :self.L].clone()[None]
        self.qval = torch.ones_like(self.kval)
        self.scale = 1.0 / math.sqrt(hd)
        self.rows, self.cols = rows, c

    def run(self, kval=None, v=None, k=None, scale=None, extra_pad=False, keep=False):
        q, k, v, dO, O = self.q, self.k if k is None else k, self.v if v is None else v, self.dO, self.O
        kval = self.kval if kval is None else kval
        qval = self.qval
        if extra_pad:
            z = torch.zeros_like(q[:, :, :1])
            q, k, v, dO, O = (torch.cat([x, z], 2) for x in (q, k, v, dO, O))
            kval = torch.cat([kval, torch.ones_like(kval[:, :1])], 1)
            qval = torch.cat([qval, torch.zeros_like(qval[:, :1])], 1)
        r = core(q, k, v, kval, qval, self.scale if scale is None else scale, self.o.f["hd"], dO=dO, O=O,
                 dlse=torch.zeros(1, 1, q.shape[2], dtype=torch.float64, device=q.device), keep=keep)
        return {key: val[0, 0][:self.L] for key, val in r.items()}


def _pick_sequence(o: Operands) -> Optional[int]:
    vis = (o.ix.kval & o.ix.qval).sum(1)
    b = int(vis.argmax())
    return b if int(vis[b]) >= 2 else None


def mutations(o: Operands, outs_f: Dict[str, torch.Tensor], outs_b: Optional[Dict[str, torch.Tensor]] = None,
              folded: Optional[bool] = None):
    """(what, phase, mutated outputs) for every mutation applicable to this call; outs_f / outs_b: passing forward / backward output
    allocations (clones are edited).  The forward mutations edit out / lse, the backward ones dqkv / dbias with the given out kept.
    folded: whether outs_b comes from a launch that folded dbias (default: not f['defer_fold'])."""
    f, ix = o.f, o.ix
    H, hd, D, R = f["H"], f["hd"], o.D, o.R
    b = _pick_sequence(o)
    if b is None or R == 0:
        return
    h = H - 1
    hdv = _Head(o, b, h, outs_f["out"])
    L, r0, rows, c = hdv.L, hdv.r0, hdv.rows, hdv.cols
    base = hdv.run(keep=True)
    colP = base["P"].sum(0)
    vis = torch.nonzero(hdv.kval[0]).flatten()
    top = vis[colP[vis].argsort(descending=True)]
    tile = slice(r0, r0 + min(16, L))

    def fwd_edit(what, r):
        t = {n: x.clone() for n, x in outs_f.items()}
        o.view("out", t["out"])[rows, c] = _bf(r["out"])
        if f["lse"]:
            lr = o.lse_rows(t["lse"]).clone()
            lr[rows, h] = r["lse"].float()
            o.set_lse_rows(lr, t["lse"])
        return what + " (forward)", "fwd", t

    def bwd_edit(what, r):
        t = {n: x.clone() for n, x in outs_b.items()}
        v = o.view("dqkv", t["dqkv"])
        for j, key in enumerate(("dq", "dk", "dv")):
            v[rows, j * D + h * hd:j * D + (h + 1) * hd] = _bf(r[key])
        return what + " (backward)", "bwd", t

    cases = []
    masked = torch.nonzero(~hdv.kval[0]).flatten()
    if masked.numel():                                                     # the masked key with the largest sum_q exp(s - lse)
        sc = (hdv.q[0, 0] @ hdv.k[0, 0].t()) * hdv.scale - base["lse"][:, None]
        alive = ~base["dead"]
        j = masked[torch.exp(sc[alive][:, masked]).sum(0).argmax()] if bool(alive.any()) else masked[0]
        kv = hdv.kval.clone()
        kv[0, j] = True
        cases.append(("one masked key let through", hdv.run(kval=kv)))
    kv = hdv.kval.clone()
    kv[0, top[0]] = False
    cases.append(("one visible key dropped", hdv.run(kval=kv)))
    v2 = hdv.v.clone()
    v2[0, 0, [int(top[0]), int(top[1])]] = hdv.v[0, 0, [int(top[1]), int(top[0])]]
    cases.append(("two V rows swapped", hdv.run(v=v2)))
    kv = hdv.kval.clone()
    kv[0, vis[-1]] = False
    cases.append(("last valid key dropped, first padding key admitted", hdv.run(kval=kv, extra_pad=True)))
    if hd == 16:
        cases.append(("scale of a 16-wide head taken as 1/sqrt(32)", hdv.run(scale=1.0 / math.sqrt(32.0))))
    for what, r in cases:
        yield fwd_edit(what, r)
        if outs_b is not None:
            yield bwd_edit(what, r)
    # ---- forward only
    if H >= 2:
        t = {n: x.clone() for n, x in outs_f.items()}
        ov = o.view("out", t["out"])
        ov[tile, c] = ov[tile, (h - 1) * hd:h * hd].clone()
        yield "one 16-row query tile taken from the neighbouring head (forward)", "fwd", t
    if f["lse"]:
        t = {n: x.clone() for n, x in outs_f.items()}
        lr = o.lse_rows(t["lse"]).clone()
        seg = lr[rows, h]
        fin = torch.where(torch.isfinite(seg), seg.abs(), torch.zeros_like(seg))
        i = int(fin.argmax())
        lr[r0 + i, h] = lr[r0 + i, h] * LOG2E
        o.set_lse_rows(lr, t["lse"])
        yield "lse of one row in log2 units (forward)", "fwd", t
    t = {n: x.clone() for n, x in outs_f.items()}
    bo = o.b["out"]
    flat = t["out"]
    src = outs_f["out"][bo.p + r0 * D:bo.p + (r0 + L) * D]
    flat[bo.p + (r0 + 1) * D:bo.p + (r0 + L + 1) * D] = src
    yield "one sequence shifted by one row (forward)", "fwd", t
    t = {n: x.clone() for n, x in outs_f.items()}
    t["out"][bo.p + R * D:bo.p + (R + 1) * D] = outs_f["out"][bo.p + (R - 1) * D:bo.p + R * D]
    yield "one row written one row past the region (forward)", "fwd", t
    if outs_b is None:
        return
    # ---- backward only
    t = {n: x.clone() for n, x in outs_b.items()}
    o.view("dqkv", t["dqkv"])[tile, h * hd:(h + 1) * hd] = _bf(base["dq"][:tile.stop - r0] / hdv.scale)
    yield "dq of one tile missing the scale factor (backward)", "bwd", t
    t = {n: x.clone() for n, x in outs_b.items()}
    wrong = base["dS"] @ hdv.q[0, 0]                                        # dS instead of dS^T
    o.view("dqkv", t["dqkv"])[tile, D + h * hd:D + (h + 1) * hd] = _bf(wrong[:tile.stop - r0])
    yield "a dk tile computed with dS^T (backward)", "bwd", t
    t = {n: x.clone() for n, x in outs_b.items()}
    bq = o.b["dqkv"]
    t["dqkv"][bq.p + R * 3 * D:bq.p + (R + 1) * 3 * D] = outs_b["dqkv"][bq.p + (R - 1) * 3 * D:bq.p + R * 3 * D]
    yield "one row written one row past the region (backward)", "bwd", t
    if f["dbias"] and ((not f["defer_fold"]) if folded is None else folded):
        t = {n: x.clone() for n, x in outs_b.items()}
        o.view("dbias", t["dbias"]).add_(o.view("dbias_ws", t["dbias_ws"])[b])
        yield "dbias_ws row of one b added twice (backward)", "bwd", t
