"""References, bounds, index patterns, mutations and an fp32 emulation for the token plumbing of csrc/misc.hip: wj_add_pos,
wj_mask_gather_rows, wj_mask_scatter_fill_pos (dense and ragged), wj_mask_scatter_fill_pos_bwd and wj_unmask_rows_f32 (test
infrastructure; used by tests/test_token_reference_cpu.py and tests/test_token_bounds_gpu.py).  The basics are those of
tests/norm_reference.py.

The forward entries are EXACT: every add is one correctly rounded fp32 add of two representable values, so an f32 output is
float32(float64(tok) + float64(pos)) bit for bit, a bf16 output is bf16 of the f32 output, a copy is a copy; the mask token is rounded
to bf16 first, as the header says.  Their references come with a bound of zero: `check` then demands equality.

Backward: dtok[m] = sum over the visible groups g of d_in[row(m, g)] in fp64, bound KAPPA u sum_g |d_in| (a chain of at most 15
additions: first order (G - 1) u sum |d_in| at the very worst, a few u for roundings that do not all fall the same way);
d_ctx_feats = bf16(dtok) on the rows with inv >= 0, through bf16_bound; the mask-token gradient and each of its partial rows (one per
workgroup of 16 token rows) are sums of such terms over their masked tokens: KAPPA u sum |term|, the terms being the d_in rows.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from tests.norm_reference import KAPPA, U, bf16, bf16_bound, f64, mutate_truncate_bf16

F = np.float32
SFB_ROWS = 16             # token rows per workgroup of the backward
Pair = Tuple[torch.Tensor, torch.Tensor]

HANDLED = {
    "wj_add_pos_args": {"x", "pos", "y_f32", "y_bf16", "M", "T", "D"},
    "wj_gather_args": {"x", "idx", "out", "n_rows", "D", "elem_bytes"},
    "wj_scatter_fill_args": {"ctx_feats", "inv", "mask_token", "pos", "rows", "out_f32", "out_bf16", "B", "T", "D", "G", "n_rows"},
    "wj_scatter_fill_bwd_args": {"d_in", "inv", "rowmap", "d_ctx_feats", "d_mask_token", "partials", "B", "T", "D", "G"},
    "wj_unmask_rows_args": {"src", "inv", "dst", "M", "D", "src_is_f32", "dst_is_bf16"},
}
EXCLUDED: Dict[str, Dict[str, str]] = {}

WIDTHS = (4, 252, 256, 260, 384, 512, 516, 768, 1020, 1024)
ROWS = (1, 15, 16, 17, 67)
GROUPS = (1, 3, 4, 5, 8, 15)
PATTERNS = ("mixed", "all_context", "all_masked", "blocks")


def exact(x: torch.Tensor) -> Pair:
    x = f64(x)
    return x, torch.zeros_like(x)


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------------------ index patterns
def split_rows(M: int) -> Tuple[int, int]:
    """(B, T) with B T = M and T no divisor of 16 where M allows it"""
    for T in (67, 17, 5, 3):
        if M % T == 0:
            return M // T, T
    return 1, M


def make_inv(pattern: str, M: int, seed: int) -> Tuple[torch.Tensor, int]:
    """(inv int32 [M]: the context row of a token or -1, n_ctx).  blocks: one workgroup's 16 rows all masked beside one all context."""
    g = _gen(seed)
    if pattern == "all_context":
        ctx = torch.ones(M, dtype=torch.bool)
    elif pattern == "all_masked":
        ctx = torch.zeros(M, dtype=torch.bool)
    else:
        ctx = torch.rand(M, generator=g) < 0.6
        ctx[0] = True               # (the ragged forms hide token 0 from every group: a context row that must receive zeros)
        if pattern == "blocks":
            ctx[:SFB_ROWS] = False
            ctx[SFB_ROWS:2 * SFB_ROWS] = True
    inv = torch.full((M,), -1, dtype=torch.int32)
    n_ctx = int(ctx.sum())
    inv[ctx] = torch.arange(n_ctx, dtype=torch.int32)
    return inv, n_ctx


def make_ragged(inv: torch.Tensor, B: int, T: int, G: int, seed: int, density: float = 0.6) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rows int32 [n]: the visible dense indices (b G + g) T + t ascending, rowmap int32 [B G T]: packed row or -1).  Token 0 is
    invisible in every group; where M > 1 the last token is visible in every group."""
    vis = torch.rand(B, G, T, generator=_gen(seed)) < density
    vis[0, :, 0] = False
    if B * T > 1:
        vis[B - 1, :, T - 1] = True
    rows = torch.nonzero(vis.reshape(-1)).squeeze(1).to(torch.int32)
    rowmap = torch.full((B * G * T,), -1, dtype=torch.int32)
    rowmap[rows.long()] = torch.arange(rows.numel(), dtype=torch.int32)
    return rows, rowmap


def dense_rows(B: int, T: int, G: int) -> torch.Tensor:
    """[B T][G]: the dense row (b G + g) T + t of token m = b T + t in group g"""
    m = torch.arange(B * T)
    b, t = m // T, m % T
    return (b[:, None] * G + torch.arange(G)[None]) * T + t[:, None]


# ------------------------------------------------------------------------------------------------------------ forward (exact)
def add_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """one correctly rounded fp32 add: float32(float64(a) + float64(b))"""
    return (f64(a) + f64(b)).float()


def add_pos(x: torch.Tensor, pos: torch.Tensor, T: int, shift: int = 0) -> Dict[str, Pair]:
    """x bf16 [M][D], pos f32 [T][D].  shift = 1: the mutation pos[t + 1]"""
    M = x.shape[0]
    y = add_f32(x, pos[(torch.arange(M) + shift) % T])
    return {"y_f32": exact(y), "y_bf16": exact(y.to(torch.bfloat16))}


def gather(x: torch.Tensor, idx: torch.Tensor) -> Pair:
    return exact(x.detach().cpu()[idx.long()])


def scatter_fill(ctx_feats, inv, mask_token, pos, B: int, T: int, G: int, rows: Optional[torch.Tensor] = None, shift: int = 0,
                 round_token: bool = True) -> Dict[str, Pair]:
    """ctx_feats bf16 [n_ctx][D], mask_token f32 [D], pos f32 [T][D]; dense [B G T][D] or, with rows, packed [n_rows][D]"""
    D = pos.shape[1]
    M = B * T
    mt = mask_token.to(torch.bfloat16).float() if round_token else mask_token.float()
    tok = mt[None].expand(M, D).clone()
    on = inv >= 0
    if ctx_feats.shape[0]:
        tok[on] = ctx_feats.float()[inv[on].long()]
    y = add_f32(tok, pos[(torch.arange(M) + shift) % T]).reshape(B, 1, T, D).expand(B, G, T, D).reshape(B * G * T, D)
    if rows is not None:
        y = y[rows.long()]
    return {"out_f32": exact(y), "out_bf16": exact(y.to(torch.bfloat16))}


def unmask(src: torch.Tensor, inv: Optional[torch.Tensor], M: int, dst_is_bf16: bool) -> Pair:
    """dst[m] = inv[m] >= 0 ? src[inv[m]] : 0; inv None: the identity.  src f32 or bf16 (widening is exact, narrowing rounds to even)"""
    s = src.detach().cpu().float()
    if inv is None:
        out = s[:M].clone()
    else:
        out = torch.zeros(M, s.shape[1])
        on = inv >= 0
        if s.shape[0]:
            out[on] = s[inv[on].long()]
    return exact(out.to(torch.bfloat16) if dst_is_bf16 else out)


# ------------------------------------------------------------------------------------------------------------ backward
def _terms(d_in, rowmap, B, T, G) -> Tuple[torch.Tensor, torch.Tensor]:
    """([M][G][D] fp64 terms with zeros where a group does not see the token, [M][G] visible)"""
    dr = dense_rows(B, T, G)
    src = dr if rowmap is None else rowmap.long()[dr]
    vis = src >= 0
    d = f64(d_in)
    t = d[src.clamp_min(0)] if d.shape[0] else torch.zeros(B * T, G, d.shape[1], dtype=torch.float64)
    return t * vis[:, :, None], vis


def scatter_fill_bwd(d_in, inv, rowmap, B: int, T: int, G: int, n_ctx: int) -> Dict[str, Pair]:
    """d_in f32 dense [B G T][D] or packed (rowmap).  d_mask_token is the sum alone (add what the buffer held); partials [ceil(M / 16)][D]"""
    terms, _ = _terms(d_in, rowmap, B, T, G)
    M, D = B * T, terms.shape[2]
    dtok = terms.sum(1)
    mag = terms.abs().sum(1)
    b_tok = KAPPA * U * mag
    on = inv >= 0
    ctx = torch.zeros(n_ctx, D, dtype=torch.float64)
    b_ctx = torch.zeros(n_ctx, D, dtype=torch.float64)
    ctx[inv[on].long()] = bf16(dtok[on])
    b_ctx[inv[on].long()] = bf16_bound(dtok[on], b_tok[on])
    off = (~on).double()[:, None]
    nwg = -(-M // SFB_ROWS)
    pad = nwg * SFB_ROWS - M
    padz = torch.zeros(pad, D, dtype=torch.float64)
    parts = torch.cat([dtok * off, padz]).reshape(nwg, SFB_ROWS, D).sum(1)
    pmag = torch.cat([mag * off, padz]).reshape(nwg, SFB_ROWS, D).sum(1)
    return {"dtok": (dtok, b_tok), "d_ctx_feats": (ctx, b_ctx), "partials": (parts, KAPPA * U * pmag),
            "d_mask_token": ((dtok * off).sum(0), KAPPA * U * (mag * off).sum(0))}


def make_d_in(kind: str, n_rows: int, D: int, seed: int, rowmap=None, B=0, T=0, G=0) -> torch.Tensor:
    """randn, or `cancel`: the groups of a token sum to nearly zero (+-1e3 alternating over the groups that see it, plus randn)"""
    x = torch.randn(n_rows, D, generator=_gen(seed))
    if kind == "randn" or n_rows == 0:
        return x
    dr = dense_rows(B, T, G)
    src = dr if rowmap is None else rowmap.long()[dr]
    for m in range(B * T):
        seen = src[m][src[m] >= 0]
        for k, row in enumerate(seen[:2 * (len(seen) // 2)].tolist()):
            x[row] += 1e3 * (1 - 2 * (k % 2))
    return x


def emulate_bwd(d_in, inv, rowmap, B: int, T: int, G: int, order: Optional[List[int]] = None) -> Dict[str, np.ndarray]:
    """scatter_fill_bwd_kernel in fp32: a token's groups in order (four at a time, the invisible ones skipped), a wave's four rows in
    order, (w0 + w1) + (w2 + w3), then the workgroups' partial rows added to the mask-token gradient in `order` (the atomic form; None:
    ascending)"""
    terms, vis = _terms(d_in, rowmap, B, T, G)
    terms = terms.numpy().astype(F)
    M, D = B * T, terms.shape[2]
    s = np.zeros((M, D), dtype=F)
    for g in range(G):
        s = np.where(vis[:, g].numpy()[:, None], (s + terms[:, g]).astype(F), s)
    on = (inv >= 0).numpy()
    nwg = -(-M // SFB_ROWS)
    wave = np.zeros((nwg * 4, D), dtype=F)
    for r in range(4):
        idx = np.arange(nwg * 4) * 4 + r
        ok = idx < M
        row = np.zeros((nwg * 4, D), dtype=F)
        live = ok.copy()
        live[ok] = ~on[idx[ok]]
        row[live] = s[idx[live]]
        wave = (wave + row).astype(F)
    w = wave.reshape(nwg, 4, D)
    parts = ((w[:, 0] + w[:, 1]).astype(F) + (w[:, 2] + w[:, 3]).astype(F)).astype(F)
    tot = np.zeros(D, dtype=F)
    for k in (range(nwg) if order is None else order):
        tot = (tot + parts[k]).astype(F)
    n_ctx = int(on.sum())
    ctx = np.zeros((n_ctx, D), dtype=F)
    ctx[inv[inv >= 0].long().numpy()] = torch.from_numpy(s[on]).to(torch.bfloat16).float().numpy()
    return {"dtok": s, "d_ctx_feats": ctx, "partials": parts, "d_mask_token": tot}


# ------------------------------------------------------------------------------------------------------------ mutations
def mutate_chunk(got, row: int, col: int, value: float = float("nan")) -> torch.Tensor:
    """the 4-column chunk at `col` of one row left stale (NaN, as the buffer was before the launch)"""
    m = f64(got).clone()
    m[row, col:col + 4] = value
    return m


def stale_columns(D: int) -> List[int]:
    """one chunk at c >= 256 and one at c >= 512, where the width has them"""
    return [c for c in (256, 512) if c + 4 <= D]


def bwd_mutations(got: Dict[str, torch.Tensor], d_in, inv, rowmap, B: int, T: int, G: int) -> List[tuple]:
    """[(label, output, mutated)] of one accepted backward: got = {d_ctx_feats [n_ctx][D] bf16, partials [nwg][D], d_mask_token [D]}.
    A mutation of a token's sum lands where that token's sum lands: its context row, or its workgroup's partial row and the total."""
    terms, vis = _terms(d_in, rowmap, B, T, G)
    M, D = B * T, terms.shape[2]
    d = f64(d_in)
    out = []

    def land(label, m, delta):
        """token m's sum moved by delta [D]"""
        if int(inv[m]) >= 0:
            x = f64(got["d_ctx_feats"]).clone()
            x[int(inv[m])] += delta
            out.append((label, "d_ctx_feats", x))
        else:
            x = f64(got["partials"]).clone()
            x[m // SFB_ROWS] += delta
            out.append((label, "partials", x))
            out.append((label, "d_mask_token", f64(got["d_mask_token"]) + delta))

    seen = [m for m in range(M) if bool(vis[m].any())]
    for m in {seen[0], seen[-1]} if seen else ():
        g = int(torch.nonzero(vis[m])[-1])
        land("a group left out", m, -terms[m, g])
        land("a group counted twice", m, terms[m, g])
    if rowmap is not None and d.shape[0]:
        hidden = [m for m in range(M) if not bool(vis[m].all())]
        for m in {hidden[0], hidden[-1]} if hidden else ():
            land("-1 in rowmap read as row 0", m, d[0] * float((~vis[m]).sum()))
    masked = [m for m in range(M) if int(inv[m]) < 0 and bool(vis[m].any())]
    if masked and got["d_ctx_feats"].shape[0]:
        x = f64(got["d_ctx_feats"]).clone()
        x[0] += terms[masked[0]].sum(0)
        out.append(("a masked row's sum routed to d_ctx_feats row 0", "d_ctx_feats", x))
    if bool(vis[M - 1].any()):
        land("the last row dropped", M - 1, -terms[M - 1].sum(0))
    for c in stale_columns(D):
        if got["d_ctx_feats"].shape[0]:
            out.append((f"chunk at column {c} stale", "d_ctx_feats", mutate_chunk(got["d_ctx_feats"], got["d_ctx_feats"].shape[0] - 1, c)))
        out.append((f"chunk at column {c} stale", "partials", mutate_chunk(got["partials"], got["partials"].shape[0] - 1, c)))
    return out


def truncated(x_f32: torch.Tensor) -> torch.Tensor:
    return mutate_truncate_bf16(x_f32)
