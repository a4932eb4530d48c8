"""The LayerNorm family, the column-sum folds, the teacher targets and the masked MSE held per element against the fp64 references and
bounds of tests/norm_reference.py (GPU only).

Every output sits NaN-filled between guard rows; every element must come back finite and within its bound, the guards untouched.
Widths: every <V, LPR> instance of the dispatch, a last chunk ending in each of the four chunk positions, one live lane.  Rows: fewer
than a wave's row slots, a dead second slot in the backward, an odd count under two rows per wave, several workgroups.  Inputs: randn,
a large common offset, one huge channel, variance far below eps, constant rows, zero rows.  At the end of an entry's test every
mutation that applies is made on the kernel's own (accepted) output and must be rejected.

With WJ_NORM_BOUNDS_REPORT=<path> the module writes one line per entry, width and input kind: the worst error / bound (and, for
instnorm_mean, the amplification kappa of its one-pass variance).
"""
import collections
import os
import time

import pytest
import torch

from tests import norm_reference as nr

pytestmark = pytest.mark.gpu

M_ONE = 9
ROWS = (1, 3, 67, 1031)
LN_CASES = [(M_ONE, D) for D in nr.WIDTHS] + [(M, D) for D in (384, 768) for M in ROWS]
# (x is bf16, with the bf16 addend r, eps): every kind runs two of them
VARIANTS = [(False, False, 1e-6), (False, True, 1e-5), (True, False, 1e-5), (True, True, 1e-6)]
GROUP_CASES = [(15, 3), (25, 5), (26, 13), (403, 201), (410, 200)]
COLSUM_BF16 = [(1, 8, 8), (31, 72, 72), (33, 200, 208), (1003, 192, 256), (4099, 64, 64)]
MSE_CASES = [(1, 1, 1, 4), (2, 3, 37, 384), (3, 4, 50, 768), (2, 2, 33, 1000)]

REPORT = collections.OrderedDict()


def note(entry, D, kind, ratio, extra=""):
    key = (entry, D, kind)
    old = REPORT.get(key, (0.0, ""))
    REPORT[key] = (max(old[0], ratio), extra or old[1])


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_NORM_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  D  input kind  worst error / bound   (tests/test_norm_bounds_gpu.py)\n")
            for (entry, D, kind), (ratio, extra) in REPORT.items():
                f.write(f"{entry:24s} D={D:<7} {kind:10s} {ratio:.3f}{'  ' + extra if extra else ''}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


def to_dev(t):
    return None if t is None else t.to(dev())


def G(M, D=None, dtype=torch.float32, fill=None):
    return nr.guarded_like(M, D, dtype, dev(), fill)


def held(entry, D, kind, got, pair, what):
    """check one output (a Guarded or a tensor) and note its ratio"""
    if isinstance(got, nr.Guarded):
        got = got.check(what)
    ratio = nr.check(got.cpu(), *pair, what=f"{entry} D={D} {kind} {what}")
    note(entry, D, kind, ratio)
    return got.cpu()


def reject_all(muts, refs, tag):
    for label, k, m in muts:
        assert nr.rejected(m, *refs[k]), f"{tag}: mutation '{label}' of {k} accepted"


# ------------------------------------------------------------------------------------------------------------ forward
def run_fwd(ops, entry, c, M, D, eps, kind, tag):
    """one checked forward launch of `entry` (+ a second one, bit-identical); returns its outputs on the CPU and the reference"""
    x, r, gamma, beta = to_dev(c["x"]), to_dev(c["r"]), to_dev(c["gamma"]), to_dev(c["beta"])
    ref = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
    outs = []
    for rep in range(2):
        y, yb, mean, rstd, s = G(M, D), G(M, D, torch.bfloat16), G(M), G(M), G(M, D)
        if entry == "layernorm_fwd":
            ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=eps, r=r, y_f32=y.view, y_bf16=yb.view, mean=mean.view, rstd=rstd.view,
                              x_is_bf16=x.dtype == torch.bfloat16)
        else:
            ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=eps, r=r, s_f32=s.view, y_f32=y.view, y_bf16=yb.view, mean=mean.view,
                                  rstd=rstd.view)
        got = {"y_f32": y, "y_bf16": yb, "mean": mean, "rstd": rstd}
        if entry == "layernorm_pre_fwd":
            got["s_f32"] = s
        if rep == 0:
            outs.append({k: held(entry, D, kind, g, ref[k], f"{k} {tag}") for k, g in got.items()})
            assert torch.equal(outs[0]["y_bf16"], outs[0]["y_f32"].to(torch.bfloat16)), f"{tag}: y_bf16 is not bf16(y_f32)"
        else:
            outs.append({k: g.check(k).cpu() for k, g in got.items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), f"{entry} {tag}: {k} differs between two launches"
    return outs[0], ref


@pytest.mark.parametrize("M,D", LN_CASES)
def test_layernorm_fwd_and_pre_fwd(ops, M, D):
    for i, kind in enumerate(nr.KINDS):
        for x_bf16, with_r, eps in (VARIANTS[i % 4], VARIANTS[(i + 2) % 4]):
            c = nr.ln_inputs(kind, M, D, 100 + i, with_r, x_bf16)
            tag = f"M={M} x_bf16={x_bf16} r={with_r} eps={eps}"
            got, ref = run_fwd(ops, "layernorm_fwd", c, M, D, eps, kind, tag)
            if M == M_ONE:      # sensitivity on the kernel's own output
                reject_all(nr.ln_fwd_mutations(c, got, eps, kind), ref, f"layernorm_fwd {kind} D={D} {tag}")
            if x_bf16:
                continue
            pre, _ = run_fwd(ops, "layernorm_pre_fwd", c, M, D, eps, kind, tag)
            if M == M_ONE:
                reject_all(nr.ln_fwd_mutations(c, pre, eps, kind), ref, f"layernorm_pre_fwd {kind} D={D} {tag}")
            # in place: s_f32 is x itself
            xin, yb = G(M, D, fill=c["x"]), G(M, D, torch.bfloat16)
            ops.layernorm_pre_fwd(xin.view, to_dev(c["gamma"]), to_dev(c["beta"]), M=M, D=D, eps=eps, r=to_dev(c["r"]), s_f32=xin.view,
                                  y_bf16=yb.view)
            held("layernorm_pre_fwd", D, kind, xin, ref["s_f32"], "s in place " + tag)
            assert torch.equal(yb.check("y_bf16 in place").cpu(), pre["y_bf16"]), tag


@pytest.mark.parametrize("D", [36, 384])
@pytest.mark.parametrize("x_bf16", [True, False])
def test_layernorm_row_remaps(ops, D, x_bf16):
    """in_seg / in_valid at P = T + 1 (padded conv token buffer), in_chan = 2 (channel-major source), the out-row remap of the backward
    with its padding rows left alone"""
    N, T, eps = 3, 10, 1e-5
    P = T + 1
    for S in (1, 2):
        M = N * S * T
        c = nr.ln_inputs("offset" if S == 1 else "randn", M, D, 300 + S, False, x_bf16)
        # tokens (n, c, t) -> buffer rows [c][n][p]
        buf = torch.full((S, N, P, D), 7.0, dtype=c["x"].dtype)
        buf[:, :, :T] = c["x"].reshape(N, S, T, D).permute(1, 0, 2, 3)
        bufd = to_dev(buf.reshape(S * N * P, D).contiguous())
        gamma, beta = to_dev(c["gamma"]), to_dev(c["beta"])
        ref = nr.layernorm_fwd(c["x"], None, c["gamma"], c["beta"], eps)
        y, yb, mean, rstd = G(M, D), G(M, D, torch.bfloat16), G(M), G(M)
        ops.layernorm_fwd(bufd, gamma, beta, M=M, D=D, eps=eps, y_f32=y.view, y_bf16=yb.view, mean=mean.view, rstd=rstd.view,
                          x_is_bf16=x_bf16, in_seg=P, in_valid=T, in_chan=S if S > 1 else 0)
        tag = f"remap S={S} x_bf16={x_bf16}"
        for k, g in (("y_f32", y), ("y_bf16", yb), ("mean", mean), ("rstd", rstd)):
            held("layernorm_fwd", D, "remap", g, ref[k], f"{k} {tag}")
        rb = nr.layernorm_bwd(c["dy"], None, c["x"], None, c["gamma"], eps)
        dsb = G(S * N * P, D, torch.bfloat16)
        ds = G(M, D)
        dg, db, dbi = (torch.zeros(D, device=dev()) for _ in range(3))
        ops.layernorm_bwd(to_dev(c["dy"]), bufd, gamma, mean.view, rstd.view, M=M, D=D, ds_f32=ds.view, ds_bf16=dsb.view, dgamma=dg, dbeta=db,
                          dbias=dbi, x_is_bf16=x_bf16, in_seg=P, in_valid=T, out_seg=P, out_valid=T, chan=S if S > 1 else 0)
        held("layernorm_bwd", D, "remap", ds, rb["ds_f32"], "ds_f32 " + tag)
        full = dsb.check("ds_bf16 " + tag).cpu().reshape(S, N, P, D)
        assert bool(torch.isnan(full[:, :, T:].float()).all()), f"{tag}: a padding row of ds_bf16 was written"
        tok = full[:, :, :T].permute(1, 0, 2, 3).reshape(M, D)
        held("layernorm_bwd", D, "remap", tok, rb["ds_bf16"], "ds_bf16 " + tag)
        held("layernorm_bwd", D, "remap", dg, rb["dgamma"], "dgamma " + tag)
        held("layernorm_bwd", D, "remap", db, rb["dbeta"], "dbeta " + tag)
        held("layernorm_bwd", D, "remap", dbi, nr.dbias(tok), "dbias " + tag)


@pytest.mark.parametrize("M,group_rows", GROUP_CASES)
def test_group_stats_of_both_forward_entries(ops, M, group_rows):
    """a group smaller than one workgroup pass, an empty last part, M no multiple of group_rows (a short last group)"""
    split = ops.GROUP_STATS_SPLIT
    assert split == nr.SPLIT
    Gn = -(-M // group_rows)
    for D in (36, 384, 1024):
        for kind in ("randn", "offset", "constant"):
            c = nr.ln_inputs(kind, M, D, 400, kind == "randn")
            if kind == "constant":
                c["x"][:] = 0.7371                  # the whole group one value: every addition of a chain rounds the same way
            x, r, gamma, beta = to_dev(c["x"]), to_dev(c["r"]), to_dev(c["gamma"]), to_dev(c["beta"])
            for entry in ("layernorm_fwd", "layernorm_pre_fwd"):
                runs = []
                for rep in range(2):
                    st, y, s = G(Gn * split, 2), G(M, D), G(M, D)
                    if entry == "layernorm_fwd":
                        ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, y_f32=y.view, group_stats=st.view, group_rows=group_rows)
                        summed = y.check("y")
                    else:
                        ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, s_f32=s.view, y_f32=y.view, group_stats=st.view,
                                              group_rows=group_rows)
                        summed = s.check("s")
                    runs.append(st.check("group_stats").cpu())
                assert torch.equal(runs[0], runs[1]), f"{entry}: group_stats differ between two launches"
                tag = f"{entry} M={M} group_rows={group_rows} D={D} {kind}"
                ref = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], 1e-6)
                held(entry, D, kind, y, ref["y_f32"], "y " + tag)
                # the sums are those of the f32 values the launch wrote (each already held to its own bound)
                gs = nr.group_stats(nr.f64(summed), None, group_rows)
                parts = runs[0].reshape(Gn, split, 2)
                held(entry + ".group_stats", D, kind, parts, gs["parts"], "parts " + tag)
                held(entry + ".group_stats", D, kind, parts.double().sum(1), gs["total"], "totals " + tag)
                if -(-group_rows // split) * (split - 1) < group_rows:       # the last part holds rows
                    assert nr.rejected(nr.mutate_drop_last_part(parts), *gs["total"]), f"{tag}: dropped part accepted"


# ------------------------------------------------------------------------------------------------------------ backward
def fold(ops, ws, rows, D, how, deterministic):
    out = torch.zeros(3, D, device=dev())
    if how == "group":
        ops.colsum_f32_group([(ws, 3 * D, rows, 3 * D, out[0], out[1], out[2], D)], deterministic=deterministic)
    else:
        ops.colsum_f32(ws, out, M=rows, N=3 * D, ldx=3 * D, deterministic=deterministic)
    return out.cpu()


def run_bwd(ops, entry, c, M, D, eps, kind, variant, tag):
    """forward (checked) -> backward in its three forms.  variant: post (dy2: None / "f32" / "bf16"), pre (dy bf16?, dres?)"""
    gamma, beta = to_dev(c["gamma"]), to_dev(c["beta"])
    x, r = to_dev(c["x"]), to_dev(c["r"])
    fref = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
    mean, rstd, s = G(M), G(M), G(M, D)
    if entry == "layernorm_bwd":
        ops.layernorm_fwd(x, gamma, beta, M=M, D=D, eps=eps, r=r, mean=mean.view, rstd=rstd.view, x_is_bf16=x.dtype == torch.bfloat16)
        dy2 = None if variant is None else (c["dy2"] if variant == "f32" else c["dy2"].to(torch.bfloat16))
        ref = nr.layernorm_bwd(c["dy"], dy2, c["x"], c["r"], c["gamma"], eps)
        dyd, dy2d = to_dev(c["dy"]), to_dev(dy2)

        def launch(**out):
            ops.layernorm_bwd(dyd, x, gamma, mean.view, rstd.view, M=M, D=D, r=r, dy2=dy2d, dy2_is_bf16=variant == "bf16",
                              x_is_bf16=x.dtype == torch.bfloat16, **out)
        rows = ops.ln_bwd_partial_rows(M, D)
    else:
        ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=eps, r=r, s_f32=s.view, mean=mean.view, rstd=rstd.view)
        held("layernorm_pre_fwd", D, kind, s, fref["s_f32"], "s " + tag)
        dy_bf16, with_dres = variant
        dy = c["dy"].to(torch.bfloat16) if dy_bf16 else c["dy"]
        dres = c["dres"] if with_dres else None
        ref = nr.layernorm_pre_bwd(dy, dres, fref["s_f32"][0].float(), c["gamma"], eps)
        dyd, dresd = to_dev(dy), to_dev(dres)

        def launch(**out):
            ops.layernorm_pre_bwd(dyd, s.view, gamma, mean.view, rstd.view, M=M, D=D, dres=dresd, dy_is_bf16=dy_bf16, **out)
        rows = ops.ln_pre_bwd_partial_rows(M, D)
    fwd_entry = "layernorm_fwd" if entry == "layernorm_bwd" else "layernorm_pre_fwd"
    held(fwd_entry, D, kind, mean, fref["mean"], "mean " + tag)
    held(fwd_entry, D, kind, rstd, fref["rstd"], "rstd " + tag)
    # form 1: atomics
    ds, dsb = G(M, D), G(M, D, torch.bfloat16)
    cols = torch.zeros(3, D, device=dev())
    launch(ds_f32=ds.view, ds_bf16=dsb.view, dgamma=cols[0], dbeta=cols[1], dbias=cols[2])
    got = {"ds_f32": held(entry, D, kind, ds, ref["ds_f32"], "ds_f32 " + tag), "ds_bf16": held(entry, D, kind, dsb, ref["ds_bf16"], "ds_bf16 " + tag)}
    assert torch.equal(got["ds_bf16"], got["ds_f32"].to(torch.bfloat16)), f"{tag}: ds_bf16 is not bf16(ds_f32)"
    ref = dict(ref, dbias=nr.dbias(got["ds_bf16"]))
    names = ("dgamma", "dbeta", "dbias")

    def hold_cols(t3, form):
        return {k: held(entry, D, kind, t3[i], ref[k], f"{k} ({form}) {tag}") for i, k in enumerate(names)}
    got.update(hold_cols(cols.cpu(), "atomic"))
    # form 2: partial rows in a workspace, folded by the entry's second kernel
    ws = G(rows * 3, D)
    cols2 = torch.zeros(3, D, device=dev())
    dsb2 = G(M, D, torch.bfloat16)
    launch(ds_bf16=dsb2.view, dgamma=cols2[0], dbeta=cols2[1], dbias=cols2[2], workspace=ws.view)
    assert torch.equal(dsb2.check("ds_bf16").cpu(), got["ds_bf16"]), tag
    ws.check("workspace " + tag)
    hold_cols(cols2.cpu(), "workspace")
    # form 3: the partial rows left in place, folded by wj_colsum_f32_group / wj_colsum_f32, atomic and in order
    ws3 = G(rows * 3, D)
    launch(ds_bf16=dsb2.view, workspace=ws3.view)
    assert bool(torch.isfinite(ws3.check("partial rows " + tag)).all()), f"{tag}: NaN left in the partial rows"
    hows = (["group"] if 3 * D <= 2304 else []) + ["single"]
    for how in hows:
        hold_cols(fold(ops, ws3.view, rows, D, how, False), f"left, {how}")
        det = []
        for _ in range(2):
            ws4 = G(rows * 3, D)
            launch(ds_bf16=dsb2.view, workspace=ws4.view)
            det.append(fold(ops, ws4.view, rows, D, how, True))
        assert torch.equal(det[0], det[1]), f"{tag}: the deterministic fold ({how}) differs between two runs"
        hold_cols(det[0], f"deterministic, {how}")
    return got, ref


@pytest.mark.parametrize("M,D", LN_CASES)
def test_layernorm_bwd_and_pre_bwd(ops, M, D):
    post = (None, "f32", "bf16")
    pre = ((False, True), (True, False), (True, True), (False, False))
    for i, kind in enumerate(nr.KINDS):
        x_bf16, with_r, eps = VARIANTS[(i + 1) % 4]
        c = nr.ln_inputs(kind, M, D, 200 + i, with_r, x_bf16)
        tag = f"M={M} x_bf16={x_bf16} r={with_r} dy2={post[i % 3]}"
        got, ref = run_bwd(ops, "layernorm_bwd", c, M, D, eps, kind, post[i % 3], tag)
        c2 = nr.ln_inputs(kind, M, D, 250 + i, not with_r)
        tag2 = f"M={M} r={not with_r} (dy_bf16, dres)={pre[i % 4]}"
        got2, ref2 = run_bwd(ops, "layernorm_pre_bwd", c2, M, D, eps, kind, pre[i % 4], tag2)
        if M == M_ONE and kind in ("randn", "offset"):
            if not x_bf16:      # bf16 rows at 1000 are small multiples of 4: narrow rows are constant and their terms vanish
                reject_all(nr.ln_bwd_mutations(got, ref["_terms"], M), ref, f"layernorm_bwd {kind} D={D}")
            reject_all(nr.ln_bwd_mutations(got2, ref2["_terms"], M), ref2, f"layernorm_pre_bwd {kind} D={D}")


# ------------------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("M,N,ldx", COLSUM_BF16)
def test_colsum_bf16(ops, M, N, ldx):
    for kind in ("randn", "cancel"):
        x = nr.colsum_input(kind, M, N, 500).to(torch.bfloat16)
        buf = torch.full((M, ldx), 3.0, dtype=torch.bfloat16)
        buf[:, :N] = x
        xd = to_dev(buf)
        out0 = torch.arange(N, dtype=torch.float32) / 8 + 1
        ref = nr.colsum_bf16(x, out0)
        out = G(1, N, fill=out0[None])
        ops.colsum_bf16(xd, out.view, M=M, N=N, ldx=ldx)
        got = held("colsum_bf16", N, kind, out, (ref[0][None], ref[1][None]), f"atomic M={M}")
        nbytes = ops.workspace_bytes("wj_colsum_bf16", M=M, N=N, deterministic=1)
        assert nbytes > 0 and nbytes % 4 == 0
        runs = []
        for _ in range(2):
            ws = torch.full((nbytes // 4 + 4,), float("nan"), device=dev())
            out = G(1, N, fill=out0[None])
            ops.colsum_bf16(xd, out.view, M=M, N=N, ldx=ldx, workspace=ws[:nbytes // 4], deterministic=True)
            runs.append(held("colsum_bf16", N, kind, out, (ref[0][None], ref[1][None]), f"deterministic M={M}"))
            assert bool(torch.isnan(ws[nbytes // 4:]).all()), "the workspace was overrun"
        assert torch.equal(runs[0], runs[1])
        assert nr.rejected(nr.mutate_colsum_row(got[0], x[M - 1], -1), *ref) and nr.rejected(nr.mutate_colsum_row(got[0], x[0], 1), *ref)


@pytest.mark.parametrize("N", [4, 132, 600])
def test_colsum_f32(ops, N):
    for kind in ("randn", "cancel"):
        for M in (1, 7, 403):
            x = nr.colsum_input(kind, M, N, 510)
            ldx = N + 4
            buf = torch.full((M, ldx), 3.0)
            buf[:, :N] = x
            out0 = torch.arange(N, dtype=torch.float32) / 8 + 1
            ref = nr.colsum_f32(x, out0)
            runs = []
            for det in (False, True, True):
                out = G(1, N, fill=out0[None])
                ops.colsum_f32(to_dev(buf), out.view, M=M, N=N, ldx=ldx, deterministic=det)
                runs.append(held("colsum_f32", N, kind, out, (ref[0][None], ref[1][None]), f"M={M} deterministic={det}"))
            assert torch.equal(runs[1], runs[2])
            assert nr.rejected(nr.mutate_colsum_row(runs[0][0], x[M - 1], -1), *ref) and nr.rejected(nr.mutate_colsum_row(runs[0][0], x[0], 1), *ref)


def test_colsum_f32_group(ops):
    """items of mixed sizes in one launch, a 128-column tile that straddles two outputs at an arbitrary column (n_each = 200), NULL
    outputs, 16 items"""
    shapes = [(1, 8, 8), (7, 2304, 768), (33, 600, 200), (403, 2304, 768), (5, 132, 44), (64, 12, 4)]
    shapes = shapes + [(3 + i, 600, 200) for i in range(ops.COLSUM_GROUP_MAX - len(shapes))]
    assert len(shapes) == 16
    for kind in ("randn", "cancel"):
        xs = [nr.colsum_input(kind, M, N, 520 + i) for i, (M, N, _) in enumerate(shapes)]
        by_run = []
        for det in (False, True, True):
            items, outs, refs = [], [], []
            for i, ((M, N, n_each), x) in enumerate(zip(shapes, xs)):
                widths = [min(n_each, max(0, N - w * n_each)) if w < 2 else max(0, N - 2 * n_each) for w in range(3)]
                o0 = [None if (wd == 0 or (i % 4 == 3 and w == 1) or (i % 4 == 1 and i > 4 and w == 2)) else torch.full((wd,), 0.5 + w)
                      for w, wd in enumerate(widths)]
                og = [None if o is None else G(1, o.numel(), fill=o[None]) for o in o0]
                ldx = N + 4 * (i % 2)
                buf = torch.full((M, ldx), 3.0)
                buf[:, :N] = x
                items.append((to_dev(buf), ldx, M, N) + tuple(None if g is None else g.view for g in og) + (n_each,))
                outs.append(og)
                refs.append(nr.colsum_f32_group(x, n_each, o0))
            ops.colsum_f32_group(items, deterministic=det)
            res = []
            for i, (og, rf) in enumerate(zip(outs, refs)):
                for w in range(3):
                    if og[w] is not None:
                        res.append(held("colsum_f32_group", shapes[i][1], kind, og[w], (rf[w][0][None], rf[w][1][None]),
                                        f"item {i} {shapes[i]} o{w} deterministic={det}"))
            by_run.append(res)
            if not det:
                # a column routed to the neighbouring output at the n_each boundary (item 2: 600 columns, n_each = 200)
                o0g, o1g = outs[2][0].view.cpu()[0], outs[2][1].view.cpu()[0]
                a, b = nr.mutate_route(o0g, o1g, float(xs[2].double()[:, 199].sum()))
                assert nr.rejected(a, *refs[2][0]) and nr.rejected(b, *refs[2][1]), "a column routed to the neighbour was accepted"
        assert all(torch.equal(a, b) for a, b in zip(by_run[1], by_run[2])), "the deterministic fold differs between two runs"


# ------------------------------------------------------------------------------------------------------------ teacher targets
@pytest.mark.parametrize("T,D,K", [(1, 4, 1), (25, 164, 8), (200, 768, 3)])
def test_instnorm_accumulate_and_mean(ops, T, D, K):
    """B = 3; layers with mean / sigma in {0, 3, 30} and one constant sample; the statistics of wj_instnorm_mean come out of
    wj_layernorm_pre_fwd (even layers: the stream itself) and wj_layernorm_fwd (odd layers: y) group_stats launches"""
    B, TD, eps = 3, T * D, 1e-5
    split = ops.GROUP_STATS_SPLIT
    raw = nr.instnorm_layers(B, TD, K, 600)
    stats = G(K * B * split, 2)
    sview = stats.view.reshape(K, B * split, 2)
    layers = []
    one, zero = torch.ones(D, device=dev()), torch.zeros(D, device=dev())
    for l, x in enumerate(raw):
        out = G(B * T, D)
        if l % 2 == 0:
            ops.layernorm_pre_fwd(to_dev(x.reshape(B * T, D)), one, zero, M=B * T, D=D, eps=1e-6, s_f32=out.view, group_stats=sview[l], group_rows=T)
        else:          # y = xh sigma + ratio sigma: the same mean / sigma out of a LayerNorm
            sig = 1.0 + 0.5 * l
            g0 = torch.Generator().manual_seed(610 + l)
            ops.layernorm_fwd(to_dev(torch.randn(B * T, D, generator=g0)), one * sig, one * (sig * nr.RATIOS[l % 3]), M=B * T, D=D, eps=1e-6,
                              y_f32=out.view, group_stats=sview[l], group_rows=T)
        layers.append(out.check(f"layer {l}").reshape(B, TD))
    xs = [x.cpu() for x in layers]
    assert all(bool(torch.isfinite(x).all()) for x in xs)
    parts = stats.check("group_stats").cpu().reshape(K, B, split, 2)
    for l, x in enumerate(xs):
        gs = nr.group_stats(nr.f64(x.reshape(B * T, D)), None, T)
        held("instnorm.group_stats", TD, f"layer{l}", parts[l], gs["parts"], f"layer {l}")
    ref = nr.instnorm_mean(xs, eps)
    kap = ref["kappa"][0]
    tg = G(B, TD)
    ops.instnorm_mean(layers, stats.view, tg.view, B=B, TD=TD, eps=eps)
    got_mean = tg.check("targets").cpu()
    for b in range(B):
        ratio = nr.check(got_mean[b], ref["targets"][0][b], ref["targets"][1][b], what=f"instnorm_mean TD={TD} K={K} sample {b}")
        note("instnorm_mean", TD, f"K={K} b={b}", ratio, "kappa " + " ".join(f"{float(k):.0f}" for k in kap[:, b]))
    # the read-twice form, layer by layer (accumulate off, then on); its running bound is the sum of the steps'
    acc = G(B, TD)
    prev, bound = None, torch.zeros(B, TD, dtype=torch.float64)
    for l, x in enumerate(layers):
        ops.instnorm_accumulate(x, acc.view, B=B, TD=TD, accumulate=l > 0, scale=1.0 / K, eps=eps)
        step = nr.instnorm_accumulate(xs[l], prev, 1.0 / K, eps)["targets"]
        prev = held("instnorm_accumulate", TD, f"K={K} layer{l}", acc, step, f"after layer {l}").clone()
        bound = bound + step[1]
    # scale = float32(1 / K) against the one-pass form's 1 / K in fp32: within u of each other, inside the 2 u |t| of the bound
    assert nr.worst(prev, got_mean.double(), bound + ref["targets"][1]) <= 1.0, "the two forms disagree beyond the sum of their bounds"
    if T > 1:
        assert nr.rejected(nr.mutate_swap_rows(got_mean, 0), *ref["targets"]), "two samples swapped accepted"
        assert nr.rejected(nr.mutate_chunk(got_mean, 1, TD // 4 - 1), *ref["targets"]), "a zero chunk accepted"


# ------------------------------------------------------------------------------------------------------------ masked MSE
def run_mse(ops, c, B, G_, T, D, tag, aligned=True, gscale=1.0, gscale_dev=None, rows=None, with_dpreds=True):
    n = B * G_ * T
    preds = c["preds"] if rows is None else (c["preds"][rows.long()] if rows.numel() else c["preds"][:1])
    R = n if rows is None else int(rows.numel())
    mbuf = torch.ones(n + 32, dtype=torch.uint8, device=dev())          # bytes around the mask are not targets of this call
    off = 0 if aligned else 1
    mbuf[off:off + n] = to_dev(c["tgt"])
    assert mbuf.data_ptr() % 16 == 0
    loss, ws = G(2), G(2 + n)
    dp = G(max(R, 1), D, torch.bfloat16)
    gp = None if gscale_dev is None else torch.tensor([gscale_dev], device=dev())
    ops.masked_mse(to_dev(preds), to_dev(c["targets"]), mbuf.data_ptr() + off, loss.view, ws.view, B=B, G=G_, T=T, D=D,
                   dpreds=dp.view if with_dpreds else None, gscale=gscale, gscale_ptr=gp,
                   rows=None if rows is None else to_dev(rows if rows.numel() else torch.zeros(1, dtype=torch.int32)), n_rows=R if rows is not None else 0)
    ref = nr.masked_mse(preds, c["targets"], c["tgt"], B, G_, T, D, gscale, gscale_dev, rows)
    ws.check("workspace " + tag)
    got = {"loss": held("masked_mse", D, tag, loss, ref["loss"], "loss " + tag)}
    if with_dpreds and R > 0:
        got["dpreds"] = held("masked_mse", D, tag, dp, ref["dpreds"], "dpreds " + tag)
        off_rows = ref["_on"][0] == 0
        assert bool((got["dpreds"][off_rows].float() == 0).all()), f"{tag}: dpreds non-zero on a row that is not a target"
    else:
        assert bool(torch.isnan(dp.check("dpreds").float()).all()), f"{tag}: dpreds written though not asked for"
    return got, ref


@pytest.mark.parametrize("B,G_,T,D", MSE_CASES)
def test_masked_mse(ops, B, G_, T, D):
    n = B * G_ * T
    c = nr.mse_inputs(B, G_, T, D, 700)
    got, ref = run_mse(ops, c, B, G_, T, D, "aligned+tail")                       # n % 16 != 0 in every case: vector path and tail
    assert n % 16 != 0
    una, _ = run_mse(ops, c, B, G_, T, D, "unaligned", aligned=False)                # the scalar fallback
    assert torch.equal(una["loss"], got["loss"]) and torch.equal(una["dpreds"], got["dpreds"])
    z, _ = run_mse(ops, nr.mse_inputs(B, G_, T, D, 701, "zeros"), B, G_, T, D, "all-zero mask")
    assert z["loss"].tolist() == [0.0, 0.0] and bool((z["dpreds"].float() == 0).all())
    o, _ = run_mse(ops, nr.mse_inputs(B, G_, T, D, 702, "ones"), B, G_, T, D, "all-ones mask")
    assert float(o["loss"][1]) == n
    run_mse(ops, c, B, G_, T, D, "gscale", gscale=0.5, gscale_dev=3.0)
    # ragged: the targets and every third of the other rows, in dense order
    on = c["tgt"] != 0
    keep = on | (torch.arange(n) % 3 == 0)
    rows = torch.nonzero(keep).squeeze(1).to(torch.int32)
    rg, _ = run_mse(ops, c, B, G_, T, D, "ragged", rows=rows)
    assert float(rg["loss"][1]) == float(got["loss"][1]) and torch.equal(rg["dpreds"], got["dpreds"][rows.long()])
    run_mse(ops, c, B, G_, T, D, "ragged, no dpreds", rows=rows, with_dpreds=False)
    e, _ = run_mse(ops, c, B, G_, T, D, "ragged, n_rows=0", rows=torch.zeros(0, dtype=torch.int32))
    assert e["loss"].tolist() == [0.0, float(on.sum())]
    # sensitivity
    assert nr.rejected(nr.mutate_count(got["loss"]), *ref["loss"]), "count off by one accepted"
    m = nr.mutate_dpreds_offrow(got["dpreds"], ref["_on"][0])
    assert m is None or nr.rejected(m, *ref["dpreds"]), "dpreds on a non-target row accepted"
    if n > 1:
        v = (nr.f64(c["preds"]) - nr.f64(c["targets"]).reshape(B, 1, T, D).expand(B, G_, T, D).reshape(n, D)) * ref["_on"][0][:, None]
        gk = 2.0 / (D * (float(on.sum()) + 1e-8))
        trunc = nr.mutate_truncate_bf16((v * gk).float())
        assert nr.rejected(trunc, *ref["dpreds"]), "truncated dpreds accepted"
