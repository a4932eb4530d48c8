"""The token plumbing (wj_add_pos, wj_mask_gather_rows, wj_mask_scatter_fill_pos dense and ragged, wj_mask_scatter_fill_pos_bwd,
wj_unmask_rows_f32) held against the references of tests/token_reference.py (GPU only).

The forward entries are exact: their outputs must be bit-equal to the reference.  The backward is held element by element to its fp64
bound, in its atomic form, as partial rows (each one against the sum of its own 16 token rows), folded through wj_colsum_f32_group, and
without the mask-token gradient.  Every output sits NaN-filled between guard rows that must come back untouched.  Widths: one live
lane, the last lane of a pass, one lane into the next pass, both JMAX instances of the backward and their boundary; rows: fewer than
one workgroup's 16, exactly 16, one more, several workgroups; groups: one pass of the four-group loop with dead slots, exactly one, a
second pass with one live group, lane 63 in use.  One case of every entry lies above its grid cap.

With WJ_TOKEN_BOUNDS_REPORT=<path> the module writes one line per entry, shape and kind with the worst error / bound, and its wall time.
"""
import collections
import ctypes
import os
import time

import pytest
import torch

from tests import norm_reference as nr
from tests import token_reference as tr

pytestmark = pytest.mark.gpu

WJ_ERR_ARG = -1                      # csrc/common.h
# every D at one (M, G), every G at D in {260, 768}, every M at D = 384
SHAPES = [(67, D, 4) for D in tr.WIDTHS] + [(67, D, G) for D in (260, 768) for G in tr.GROUPS] + [(M, 384, 5) for M in tr.ROWS]
ROW_SHAPES = [(67, D) for D in tr.WIDTHS] + [(M, 384) for M in tr.ROWS if M != 67]

REPORT = collections.OrderedDict()


def note(entry, shape, kind, ratio):
    key = (entry, shape, kind)
    REPORT[key] = max(REPORT.get(key, 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_TOKEN_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  shape  kind  worst error / bound (0: bit-equal)   (tests/test_token_bounds_gpu.py)\n")
            for (entry, shape, kind), ratio in REPORT.items():
                f.write(f"{entry:34s} {shape:22s} {kind:28s} {ratio:.3f}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


def to_dev(t):
    return None if t is None else t.to(dev())


def G(M, D, dtype=torch.float32, fill=None):
    return nr.guarded_like(M, D, dtype, dev(), fill)


def ptr(g):
    """the address of a guarded view, also of an empty one (a tensor without elements reports no address)"""
    return g.buf.data_ptr() + nr.GUARD * g.buf.shape[1] * g.buf.element_size()


def held(entry, shape, kind, got, pair, what):
    if isinstance(got, nr.Guarded):
        got = got.check(f"{entry} {shape} {kind} {what}")
    got = got.cpu()
    ratio = nr.check(got, *pair, what=f"{entry} {shape} {kind} {what}")
    note(entry, shape, kind, ratio)
    return got


def untouched(g, what):
    assert bool(torch.isnan(g.check(what).float()).all()), f"{what}: written though not asked for"


def inputs(M, D, n_ctx, T, seed):
    gen = torch.Generator().manual_seed(seed)
    feats = torch.randn(max(n_ctx, 1), D, generator=gen).to(torch.bfloat16)[:n_ctx]
    return feats, 0.02 * torch.randn(D, generator=gen), torch.randn(T, D, generator=gen)


def feats_dev(feats, D):
    """the context features on the device: never a NULL pointer, also without a row"""
    return to_dev(feats) if feats.shape[0] else torch.zeros(1, D, dtype=torch.bfloat16, device=dev())


# ------------------------------------------------------------------------------------------------------------ add_pos
def run_add_pos(ops, x, pos, M, T, D, tag):
    ref = tr.add_pos(x, pos, T)
    xd, pd = to_dev(x), to_dev(pos)
    for want in (("y_f32", "y_bf16"), ("y_f32",), ("y_bf16",)):
        y, yb = G(M, D), G(M, D, torch.bfloat16)
        ops.add_pos(xd, pd, M=M, T=T, D=D, y_f32=y.view if "y_f32" in want else None, y_bf16=yb.view if "y_bf16" in want else None)
        for k, g in (("y_f32", y), ("y_bf16", yb)):
            if k in want:
                got = held("add_pos." + k, tag, "+".join(want), g, ref[k], "")
            else:
                untouched(g, f"add_pos {tag} {k}")
    return got, ref


@pytest.mark.parametrize("M,D", ROW_SHAPES)
def test_add_pos(ops, M, D):
    B, T = tr.split_rows(M)
    gen = torch.Generator().manual_seed(200)
    x, pos = torch.randn(M, D, generator=gen).to(torch.bfloat16), torch.randn(T, D, generator=gen)
    _, ref = run_add_pos(ops, x, pos, M, T, D, f"M={M} D={D}")
    if T > 1:
        assert nr.rejected(tr.add_pos(x, pos, T, shift=1)["y_f32"][0], *ref["y_f32"]), "pos[t + 1] accepted"
    assert nr.rejected(tr.truncated(ref["y_f32"][0].float()), *ref["y_bf16"]), "truncated bf16 accepted"
    assert nr.rejected(tr.mutate_chunk(ref["y_f32"][0], M - 1, D - 4), *ref["y_f32"])


def test_add_pos_and_unmask_above_the_grid_cap(ops):
    """M D / 4 > 8192 x 256: the grid-stride loops make a second pass"""
    M, D, T = 8200, 1024, 67
    assert M * D // 4 > 8192 * 256
    gen = torch.Generator().manual_seed(201)
    x, pos = torch.randn(M, D, generator=gen).to(torch.bfloat16), torch.randn(T, D, generator=gen)
    ref = tr.add_pos(x, pos, T)
    y, yb = G(M, D), G(M, D, torch.bfloat16)
    ops.add_pos(to_dev(x), to_dev(pos), M=M, T=T, D=D, y_f32=y.view, y_bf16=yb.view)
    held("add_pos.y_f32", f"M={M} D={D}", "above the cap", y, ref["y_f32"], "")
    held("add_pos.y_bf16", f"M={M} D={D}", "above the cap", yb, ref["y_bf16"], "")
    inv, n_ctx = tr.make_inv("mixed", M, 202)
    dst = G(M, D)
    ops.unmask_rows_f32(to_dev(x[:n_ctx].contiguous()), to_dev(inv), dst.view, M=M, D=D)
    held("unmask_rows_f32", f"M={M} D={D}", "above the cap", dst, tr.unmask(x[:n_ctx], inv, M, False), "")


# ------------------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("M,D", ROW_SHAPES + [(20000, 8)])
def test_mask_gather_rows(ops, M, D):
    """elem_bytes 2 and 4; n_rows = 0; (20000, 8): 16390 listed rows, above the cap of 16384 workgroups"""
    gen = torch.Generator().manual_seed(210)
    keep = torch.rand(M, generator=gen) < 0.5
    keep[M - 1] = True
    idx = torch.nonzero(keep).squeeze(1).to(torch.int32)
    if M == 20000:
        idx = torch.randperm(M, generator=gen)[:16390].sort().values.to(torch.int32)
    n = int(idx.numel())
    for eb, dtype in ((4, torch.float32), (2, torch.bfloat16)):
        if (D * eb) & 15:
            continue
        x = torch.randn(M, D, generator=gen).to(dtype)
        out = G(n, D, dtype)
        ops.mask_gather_rows(to_dev(x), to_dev(idx), out.view, n_rows=n, D=D, elem_bytes=eb)
        ref = tr.gather(x, idx)
        held("mask_gather_rows", f"M={M} D={D}", f"elem_bytes={eb}", out, ref, f"n_rows={n}")
        if n > 1:
            assert nr.rejected(nr.mutate_swap_rows(ref[0], n - 2), *ref) and nr.rejected(tr.mutate_chunk(ref[0], n - 1, D - 4), *ref)
        none = G(1, D, dtype)
        ops.mask_gather_rows(to_dev(x), to_dev(idx), none.view, n_rows=0, D=D, elem_bytes=eb)
        untouched(none, "gather of no row")


# ------------------------------------------------------------------------------------------------------------ scatter
def run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, rows, tag, kind, outputs=(("out_f32", "out_bf16"), ("out_f32",), ("out_bf16",))):
    ref = tr.scatter_fill(feats, inv, mtok, pos, B, T, Gn, rows)
    R = B * Gn * T if rows is None else int(rows.numel())
    fd, invd, md, pd = feats_dev(feats, D), to_dev(inv), to_dev(mtok), to_dev(pos)
    rd = None if rows is None else (to_dev(rows) if R else torch.zeros(1, dtype=torch.int32, device=dev()))
    for want in outputs:
        o32, o16 = G(R, D), G(R, D, torch.bfloat16)
        ops.mask_scatter_fill_pos(fd, invd, md, pd, B=B, T=T, D=D, G=Gn, out_f32=ptr(o32) if "out_f32" in want else None,
                                  out_bf16=ptr(o16) if "out_bf16" in want else None, rows=rd, n_rows=R if rows is not None else 0)
        for k, g in (("out_f32", o32), ("out_bf16", o16)):
            if k in want:
                held("scatter_fill_pos." + k, tag, kind, g, ref[k], "+".join(want))
            else:
                untouched(g, f"scatter {tag} {k}")
    return ref


@pytest.mark.parametrize("M,D,Gn", SHAPES)
def test_mask_scatter_fill_pos_dense_and_ragged(ops, M, D, Gn):
    B, T = tr.split_rows(M)
    tag = f"M={M} D={D} G={Gn}"
    for i, pattern in enumerate(tr.PATTERNS):
        inv, n_ctx = tr.make_inv(pattern, M, 220 + i)
        feats, mtok, pos = inputs(M, D, n_ctx, T, 230 + i)
        ref = run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, None, tag, pattern)
        rows, _ = tr.make_ragged(inv, B, T, Gn, 240 + i)
        rr = run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, rows, tag, pattern + ", ragged")
        assert torch.equal(rr["out_f32"][0], ref["out_f32"][0][rows.long()])
        for short in (rows[:0], rows[-1:]):                                 # lists of length 0 and 1
            run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, short, tag, pattern + ", ragged", outputs=(("out_f32", "out_bf16"),))
        if pattern == "mixed":
            for k in ("out_f32", "out_bf16"):
                if T > 1:
                    assert nr.rejected(tr.scatter_fill(feats, inv, mtok, pos, B, T, Gn, shift=1)[k][0], *ref[k]), f"{tag}: pos[t + 1] accepted"
                # (claimed on the f32 output alone: 2^-9 of a token of 0.02 moves a bf16 sum of order 1 on a fraction of a percent of
                #  the elements, which a narrow case may not hold)
                if n_ctx < M and k == "out_f32":
                    assert nr.rejected(tr.scatter_fill(feats, inv, mtok, pos, B, T, Gn, round_token=False)[k][0], *ref[k]), \
                        f"{tag}: a mask token that was not rounded to bf16 accepted"
                for c in tr.stale_columns(D):
                    assert nr.rejected(tr.mutate_chunk(ref[k][0], M * Gn - 1, c), *ref[k]), f"{tag}: stale chunk at {c} accepted"
            assert nr.rejected(tr.truncated(ref["out_f32"][0].float()), *ref["out_bf16"]), f"{tag}: truncated bf16 accepted"


def test_mask_scatter_fill_pos_above_the_grid_cap(ops):
    """B T = 32771 > 8192 workgroups x 4 rows, dense and ragged"""
    B, T, D, Gn = 1, 32771, 4, 1
    inv, n_ctx = tr.make_inv("mixed", B * T, 250)
    feats, mtok, pos = inputs(B * T, D, n_ctx, T, 251)
    one = (("out_f32", "out_bf16"),)
    run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, None, "B T=32771 D=4 G=1", "above the cap", outputs=one)
    rows = torch.arange(B * T, dtype=torch.int32)
    run_scatter(ops, feats, inv, mtok, pos, B, T, D, Gn, rows, "B T=32771 D=4 G=1", "above the cap, ragged", outputs=one)


# ------------------------------------------------------------------------------------------------------------ scatter backward
def run_bwd(ops, d_in, inv, rowmap, B, T, D, Gn, n_ctx, tag, kind, pattern):
    """one case in the four forms; the report keeps the worst ratio over the index patterns per (shape, dense / ragged, d_in kind)"""
    ref = tr.scatter_fill_bwd(d_in, inv, rowmap, B, T, Gn, n_ctx)
    M = B * T
    dd = to_dev(d_in) if d_in.shape[0] else torch.zeros(1, D, device=dev())
    invd, rmd = to_dev(inv), to_dev(rowmap)
    nwg = ops.scatter_fill_bwd_partial_rows(B, T)
    assert nwg == ref["partials"][0].shape[0]
    assert ops.workspace_bytes("wj_mask_scatter_fill_pos_bwd", B=B, T=T, D=D, G=Gn) == nwg * D * 4
    start = 0.25 * torch.arange(D, dtype=torch.float32)

    def launch(with_token, with_partials):
        ctx, tok, part = G(n_ctx, D, torch.bfloat16), G(1, D, fill=start[None]), G(nwg, D)
        ops.mask_scatter_fill_pos_bwd(dd, invd, ptr(ctx), tok.view if with_token else None, B=B, T=T, D=D, G=Gn, rowmap=rmd,
                                      partials=part.view if with_partials else None)
        return ctx, tok, part

    tok_pair = (ref["d_mask_token"][0] + start.double(), ref["d_mask_token"][1] + nr.KAPPA * nr.U * start.double())
    got = {}
    # the atomic form
    ctx, tok, part = launch(True, False)
    got["d_ctx_feats"] = held("scatter_fill_pos_bwd.d_ctx_feats", tag, kind, ctx, ref["d_ctx_feats"], pattern + ", atomic form")
    held("scatter_fill_pos_bwd.d_mask_token", tag, kind + ", atomic", tok.check("d_mask_token")[0], tok_pair, pattern + ", atomic form")
    untouched(part, f"{tag}: partials in the atomic form")
    # partial rows: two launches bit-identical, d_mask_token untouched, then folded
    runs = []
    for _ in range(2):
        ctx, tok, part = launch(True, True)
        assert torch.equal(ctx.check("d_ctx_feats").cpu(), got["d_ctx_feats"]), f"{tag}: d_ctx_feats differs between the forms"
        assert torch.equal(tok.check("d_mask_token").cpu()[0], start), f"{tag}: d_mask_token written beside partials"
        runs.append(held("scatter_fill_pos_bwd.partials", tag, kind, part, ref["partials"], pattern + ", partial rows"))
        ops.colsum_f32_group([(part.view, D, nwg, D, tok.view, None, None, D)])
        held("scatter_fill_pos_bwd.d_mask_token", tag, kind + ", folded", tok.check("folded")[0], tok_pair, pattern + ", colsum_f32_group")
    assert torch.equal(runs[0], runs[1]), f"{tag}: the partial rows differ between two launches"
    got["partials"] = runs[0]
    got["d_mask_token"] = tok.view.cpu()[0].double() - start.double()
    # without the mask-token gradient
    ctx, tok, part = launch(False, True)
    assert torch.equal(ctx.check("d_ctx_feats").cpu(), got["d_ctx_feats"]), f"{tag}: d_ctx_feats differs without d_mask_token"
    untouched(part, f"{tag}: partials without d_mask_token")
    assert torch.equal(tok.check("d_mask_token").cpu()[0], start)
    return got, ref


@pytest.mark.parametrize("M,D,Gn", SHAPES)
def test_mask_scatter_fill_pos_bwd(ops, M, D, Gn):
    B, T = tr.split_rows(M)
    tag = f"M={M} D={D} G={Gn}"
    for i, pattern in enumerate(tr.PATTERNS):
        inv, n_ctx = tr.make_inv(pattern, M, 260 + i)
        for ragged in (False, True):
            rows, rowmap = tr.make_ragged(inv, B, T, Gn, 270 + i) if ragged else (None, None)
            n_in = B * Gn * T if rows is None else int(rows.numel())
            for kind in ("randn", "cancel"):
                d_in = tr.make_d_in(kind, n_in, D, 280 + i, rowmap, B, T, Gn)
                label = f"{pattern}{', ragged' if ragged else ''}, {kind}"
                got, ref = run_bwd(ops, d_in, inv, rowmap, B, T, D, Gn, n_ctx, tag, f"{'ragged' if ragged else 'dense'}, {kind}", pattern)
                if pattern in ("mixed", "blocks"):
                    for name, k, m in tr.bwd_mutations(got, d_in, inv, rowmap, B, T, Gn):
                        assert nr.rejected(m, *ref[k]), f"{tag} {label}: mutation '{name}' of {k} accepted"
                    on = inv >= 0
                    if n_in and bool(on.any()) and not (ragged and M == 1):
                        pair = (ref["d_ctx_feats"][0][inv[on].long()], ref["d_ctx_feats"][1][inv[on].long()])
                        assert nr.rejected(tr.truncated(ref["dtok"][0][on].float()), *pair), f"{tag} {label}: truncated d_ctx_feats accepted"


# ------------------------------------------------------------------------------------------------------------ unmask
@pytest.mark.parametrize("M,D", ROW_SHAPES)
def test_unmask_rows(ops, M, D):
    """all four dtype combinations, inv = NULL, every index pattern"""
    gen = torch.Generator().manual_seed(290)
    for i, pattern in enumerate(tr.PATTERNS):
        inv, n_ctx = tr.make_inv(pattern, M, 291 + i)
        src32 = torch.randn(max(n_ctx, 1), D, generator=gen)[:n_ctx]
        for src_f32 in (False, True):
            src = src32 if src_f32 else src32.to(torch.bfloat16)
            sd = to_dev(src) if n_ctx else torch.zeros(1, D, dtype=src.dtype, device=dev())
            for dst_bf16 in (False, True):
                dst = G(M, D, torch.bfloat16 if dst_bf16 else torch.float32)
                ops.unmask_rows_f32(sd, to_dev(inv), dst.view, M=M, D=D, src_is_f32=src_f32, dst_is_bf16=dst_bf16)
                ref = tr.unmask(src, inv, M, dst_bf16)
                held("unmask_rows_f32", f"M={M} D={D}", pattern, dst, ref, f"f32 src={src_f32}, bf16 dst={dst_bf16}")
                if pattern == "mixed" and src_f32 and dst_bf16 and n_ctx:
                    wide = tr.unmask(src, inv, M, False)[0].float()
                    assert nr.rejected(tr.truncated(wide), *ref), "truncated bf16 accepted"
                if n_ctx:
                    ident = G(n_ctx, D, torch.bfloat16 if dst_bf16 else torch.float32)
                    ops.unmask_rows_f32(sd, None, ident.view, M=n_ctx, D=D, src_is_f32=src_f32, dst_is_bf16=dst_bf16)
                    held("unmask_rows_f32", f"M={M} D={D}", "identity", ident, tr.unmask(src, None, n_ctx, dst_bf16),
                         f"f32 src={src_f32}, bf16 dst={dst_bf16}")


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(ops):
    """G = 0, G = 16 and D = 1028 (backward), D & 3, D elem_bytes & 15 (gather): WJ_ERR_ARG, and no buffer is written"""
    from wavjepa_amd import _abi
    lib = _abi.load()
    stream = torch.cuda.current_stream().cuda_stream
    B, T, D, Gn = 2, 17, 1028, 16
    outs = {k: G(B * Gn * T, D) for k in ("a", "b", "c")}
    idx = torch.zeros(B * Gn * T, dtype=torch.int32, device=dev())
    src = torch.zeros(B * Gn * T, D, device=dev())
    p = {k: g.view.data_ptr() for k, g in outs.items()}

    def rc(fn, struct, **fields):
        return getattr(lib, fn)(ctypes.byref(_abi.STRUCTS[struct](**fields)), stream)

    bwd = dict(d_in=src.data_ptr(), inv=idx.data_ptr(), rowmap=0, d_ctx_feats=p["a"], d_mask_token=p["b"], partials=p["c"], B=B, T=T, D=384, G=4)
    for bad in [dict(G=0), dict(G=16), dict(D=1028), dict(D=386), dict(D=0), dict(B=0), dict(d_in=0), dict(inv=0), dict(d_ctx_feats=0)]:
        assert rc("wj_mask_scatter_fill_pos_bwd", "wj_scatter_fill_bwd_args", **{**bwd, **bad}) == WJ_ERR_ARG, bad
    fwd = dict(ctx_feats=src.data_ptr(), inv=idx.data_ptr(), mask_token=src.data_ptr(), pos=src.data_ptr(), rows=0, out_f32=p["a"], out_bf16=p["b"],
               B=B, T=T, D=384, G=4, n_rows=0)
    for bad in [dict(G=0), dict(D=386), dict(D=0), dict(T=0), dict(ctx_feats=0), dict(inv=0), dict(mask_token=0), dict(pos=0),
                dict(rows=idx.data_ptr(), n_rows=-1)]:
        assert rc("wj_mask_scatter_fill_pos", "wj_scatter_fill_args", **{**fwd, **bad}) == WJ_ERR_ARG, bad
    gat = dict(x=src.data_ptr(), idx=idx.data_ptr(), out=p["a"], n_rows=4, D=8, elem_bytes=4)
    for bad in [dict(D=4, elem_bytes=2), dict(D=6, elem_bytes=4), dict(D=12, elem_bytes=2), dict(elem_bytes=3), dict(elem_bytes=8), dict(n_rows=-1),
                dict(D=0), dict(x=0), dict(idx=0), dict(out=0)]:
        assert rc("wj_mask_gather_rows", "wj_gather_args", **{**gat, **bad}) == WJ_ERR_ARG, bad
    add = dict(x=src.data_ptr(), pos=src.data_ptr(), y_f32=p["a"], y_bf16=p["b"], M=4, T=2, D=8)
    for bad in [dict(D=6), dict(D=0), dict(M=0), dict(T=0), dict(x=0), dict(pos=0)]:
        assert rc("wj_add_pos", "wj_add_pos_args", **{**add, **bad}) == WJ_ERR_ARG, bad
    unm = dict(src=src.data_ptr(), inv=idx.data_ptr(), dst=p["a"], M=4, D=8, src_is_f32=1, dst_is_bf16=0)
    for bad in [dict(D=6), dict(D=0), dict(M=0), dict(src=0), dict(dst=0)]:
        assert rc("wj_unmask_rows_f32", "wj_unmask_rows_args", **{**unm, **bad}) == WJ_ERR_ARG, bad
    torch.cuda.synchronize()
    for k, g in outs.items():
        untouched(g, f"a refused call wrote buffer {k}")
