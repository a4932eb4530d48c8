"""The conv layer 0 reference helper (tests/conv0_reference.py) on the host.

  * its fp64 reference agrees with torch float64: F.conv1d -> F.group_norm -> F.gelu and its autograd, the bf16 rounding of the conv
    output straight-through, the accumulators' initial contents added (1e-12);
  * an fp32 numpy emulation in the kernels' documented order stays below MARGIN of every bound on every input kind and every shape the
    GPU test uses (tests/conv0_reference.py holds the tables) -- the margin of the bounds, measured on the reference side only, printed;
  * every mutation of the emulation's output is rejected at the smallest shape where it applies, the unmutated output is accepted;
  * stats_form's chunk count equals the library's workspace query over a grid of (N, C_in, C, L_out);
  * the argument errors of both entry points are answered before a launch (no GPU needed);
  * every field of the two argument structs is handled by the reference.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv0_reference as cr
from tests.test_norm_reference_cpu import MARGIN
from wavjepa_amd import _abi

W = collections.defaultdict(float)
KAPPA_SEEN = collections.defaultdict(float)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ torch float64
@pytest.mark.parametrize("C_in,lists", [(1, None), (2, None), (1, [[0, 3, 17], [], [5], list(range(20))])])
def test_reference_agrees_with_torch_float64(C_in, lists):
    N, C, L_out = 4, 16, 20
    c = cr.make_case("randn", N, C_in, L_out, C, 3, tail=3)
    geo = c["geometry"]
    wr = c["w"].double().requires_grad_(True)
    gr, br = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    yu = F.conv1d(c["audio"].double(), wr, stride=geo["stride"])
    assert yu.shape[2] == L_out
    y = yu + (cr.bf16(yu.detach()) - yu).detach()
    z = F.gelu(F.group_norm(y, C, gr, br, cr.f32eps(c["eps"]))).transpose(1, 2)
    fw = cr.conv0_fwd(c["audio"], c["w"], c["gamma"], c["beta"], c["eps"], geo, "fallback")
    assert rel(fw["act"][0][:, :L_out], cr.bf16(z.detach())) < 1e-12 and float(fw["act"][0][:, L_out:].abs().max()) == 0.0
    yd = y.detach()
    assert rel(fw["mean"][0], yd.mean(2)) < 1e-12
    assert rel(fw["rstd"][0], torch.rsqrt(yd.var(2, unbiased=False) + cr.f32eps(c["eps"]))) < 1e-12
    # the Gram form: the statistics of the unrounded conv output
    fg = cr.conv0_fwd(c["audio"], c["w"], c["gamma"], c["beta"], c["eps"], geo, "gram")
    assert rel(fg["mean"][0], yu.detach().mean(2)) < 1e-12
    assert rel(fg["rstd"][0], torch.rsqrt(yu.detach().var(2, unbiased=False) + cr.f32eps(c["eps"]))) < 1e-12
    X = cr.patches(c["audio"], geo["k"], geo["stride"], L_out)
    assert rel(fg["yx"][0], torch.einsum("nct,ntq->ncq", yu.detach(), X)) < 1e-12 and rel(fg["x1"][0], X.sum(1)) < 1e-12
    # backward: autograd, the unlisted rows with zero gradient, += into the accumulators
    dact = cr.make_dact(c, 4)
    d = torch.nan_to_num(dact.double())[:, :L_out] * cr.live_mask(N, L_out, lists).double()[:, :, None]
    z.backward(d)
    g = torch.Generator().manual_seed(5)
    dw0, dg0, db0 = torch.randn(C, C_in * geo["k"], generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    bw = cr.conv0_bwd(c["audio"], c["w"], c["gamma"], c["beta"], fw["mean"][0], fw["rstd"][0], fw["yx"][0], fw["x1"][0], dact, geo, lists,
                      dw0, dg0, db0)
    assert rel(bw["dw"][0], dw0.double() + wr.grad.reshape(C, -1)) < 1e-12
    assert rel(bw["dgamma"][0], dg0.double() + gr.grad) < 1e-12 and rel(bw["dbeta"][0], db0.double() + br.grad) < 1e-12


# ------------------------------------------------------------------------------------------------------------ margin
def hold(name, got, pair):
    r = cr.worst(t(got) if isinstance(got, np.ndarray) else got, *pair)
    W[name] = max(W[name], r)
    return r


def fwd_emulated(case, form):
    emu = cr.emulate_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], case["geometry"], form)
    ref = cr.conv0_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], case["geometry"], form)
    return emu, ref


def own_y(emu, ref):
    """None when the emulation rounded every conv output to the bf16 value the reference did.  Else its y: where the fp32 sum lies on the
    other side of a rounding boundary the error is the straddle interval of the bound itself, attained exactly; the margin of the
    ACCUMULATION terms is then measured against the bound at the emulation's own y (and the general bound must still hold, at 1)."""
    y = t(emu["_y"]).double()
    return None if torch.equal(y, ref["_y"][0]) else y


def hold_fwd(tag, case, form, cls):
    emu, ref = fwd_emulated(case, form)
    y = own_y(emu, ref)
    own = ref if y is None else cr.conv0_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], case["geometry"], form, y=y)
    for k in ("act", "mean", "rstd", "yx", "x1"):
        cr.check(t(emu[k]), *ref[k], what=f"{tag}: {k}")
        r = hold(f"fwd {k} [{form['form']}]", emu[k], own[k])
        assert r < MARGIN, f"{tag}: {k} emulation / bound = {r:.3f}"
    if case["geometry"]["L_out"] > 1:                       # one time step: var = 0, kappa = y^2 / eps whatever the input
        KAPPA_SEEN[case["kind"]] = max(KAPPA_SEEN[case["kind"]], float(ref["kappa"][0].max()))
        if case["kind"] == "offset":
            assert float(ref["kappa"][0].max()) >= 100, tag
    return emu, ref


def bwd_emulated(case, emu, lists, init, seed, margin_of=None):
    geo = case["geometry"]
    dact = cr.make_dact(case, seed)
    if lists is not None:
        dact = cr.mask_unlisted(dact, lists, geo["L_out"])
    C, Tn = case["C"], case["C_in"] * geo["k"]
    g = torch.Generator().manual_seed(seed + 1)
    zero = [None] * 3
    inits = [torch.randn(C, Tn, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)] if init else zero
    st = [t(emu[k]) for k in ("mean", "rstd", "yx", "x1")]
    got = cr.emulate_bwd(case["audio"], case["w"], case["gamma"], case["beta"], *st, dact, geo, lists, *inits)
    ref = cr.conv0_bwd(case["audio"], case["w"], case["gamma"], case["beta"], *st, dact, geo, lists, *inits)
    y = own_y(got, ref["_ctx"] and {"_y": (ref["_ctx"]["y"],)})
    got.pop("_y")
    if margin_of is not None:
        own = ref if y is None else cr.conv0_bwd(case["audio"], case["w"], case["gamma"], case["beta"], *st, dact, geo, lists, *inits, y=y)
        for k in ("dw", "dgamma", "dbeta"):
            cr.check(t(got[k]), *ref[k], what=f"{margin_of}: {k}")
            r = hold(f"bwd {k} {'dense' if lists is None else 'listed'}", got[k], own[k])
            assert r < MARGIN, f"{margin_of}: {k} emulation / bound = {r:.3f}"
    return got, ref


@pytest.mark.parametrize("table", ["FWD_EDGES", "FWD_TWO_CHANNELS", "FWD_WIDE", "FWD_LONG"])
def test_forward_emulation_stays_below_the_margin(table):
    for i, (N, C_in, C, L_out, pad, tail, kinds) in enumerate(getattr(cr, table)):
        form = cr.stats_form(N, C_in, C, L_out)
        for j, kind in enumerate(kinds):
            case = cr.make_case(kind, N, C_in, L_out, C, 100 + 10 * i + j, tail=tail, pad=pad)
            hold_fwd(f"{table} C_in={C_in} C={C} L_out={L_out} {kind}", case, form, table)


def test_forward_emulation_of_the_long_statistics_chunks():
    for N, distinct, C_in, C, L_out in cr.FWD_LONG_CHUNKS:
        form = cr.stats_form(N, C_in, C, L_out)
        assert form["form"] == "gram" and form["tcs"] == (2112 if C_in == 1 else 1088)
        for kind in ("randn", "offset"):
            hold_fwd(f"long chunks C_in={C_in} {kind}", cr.make_case(kind, distinct, C_in, L_out, C, 300), form, "FWD_LONG_CHUNKS")


def test_forward_emulation_of_the_strided_batch():
    for N, C, L_out in cr.STRIDED:
        both = cr.make_case("randn", N, 2, L_out, C, 350, tail=3)
        for c in range(2):
            case = dict(both, audio=both["audio"][:, c:c + 1].contiguous(), C_in=1, w=both["w"][:, c:c + 1].contiguous())
            hold_fwd(f"strided C={C} channel {c}", case, cr.stats_form(N, 1, C, L_out), "STRIDED")


def test_both_statistics_forms_and_both_apply_forms_are_reached():
    forms = collections.Counter()
    for table in (cr.FWD_EDGES, cr.FWD_TWO_CHANNELS, cr.FWD_WIDE, cr.FWD_LONG):
        for N, C_in, C, L_out, pad, tail, kinds in table:
            f = cr.stats_form(N, C_in, C, L_out)
            forms[(f["form"], cr.apply_form(C), C_in, min(f["chunks"], 2))] += 1
    for key in (("gram", "mfma", 1, 1), ("gram", "mfma", 1, 2), ("gram", "valu", 1, 1), ("fallback", "valu", 1, 1), ("fallback", "valu", 1, 2),
                ("fallback", "mfma", 2, 1), ("gram", "mfma", 2, 2), ("gram", "valu", 2, 1), ("fallback", "valu", 2, 2)):
        assert forms[key], key
    # the two forms differ by far more than the bound of either at short L_out: a GPU run in the wrong form cannot pass
    case = cr.make_case("randn", 3, 1, 17, 64, 7)
    a = cr.conv0_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], case["geometry"], "gram")
    b = cr.conv0_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], case["geometry"], "fallback")
    assert cr.rejected(a["mean"][0], *b["mean"]) and cr.rejected(b["mean"][0], *a["mean"])
    assert cr.rejected(a["yx"][0], *b["yx"]) and cr.rejected(b["yx"][0], *a["yx"])


@pytest.mark.parametrize("idx", range(len(cr.BWD_DENSE)))
def test_dense_backward_emulation_stays_below_the_margin(idx):
    N, C_in, C, L_out, kinds = cr.BWD_DENSE[idx]
    form = cr.stats_form(N, C_in, C, L_out)
    for j, kind in enumerate(kinds):
        case = cr.make_case(kind, N, C_in, L_out, C, 400 + 10 * idx + j)
        emu, _ = hold_fwd(f"bwd dense {idx} {kind}", case, form, "BWD_DENSE")
        for init in (False, True):
            bwd_emulated(case, emu, None, init, 500 + idx, margin_of=f"dense {idx} {kind} init={init}")


@pytest.mark.parametrize("idx", range(len(cr.BWD_LISTED)))
def test_listed_backward_emulation_stays_below_the_margin(idx):
    counts, _, kinds = cr.BWD_LISTED[idx]
    N, L_out = len(counts), cr.BWD_LISTED_L_OUT
    form = cr.stats_form(N, 1, 64, L_out)
    lists = cr.make_lists(counts, L_out, 600 + idx)
    assert [len(tl) for tl in lists] == counts
    for j, kind in enumerate(kinds):
        case = cr.make_case(kind, N, 1, L_out, 64, 610 + 10 * idx + j)
        emu, _ = hold_fwd(f"bwd listed {idx} {kind}", case, form, "BWD_LISTED")
        bwd_emulated(case, emu, lists, True, 700 + idx, margin_of=f"listed {idx} {kind}")


def test_zz_report_of_the_worst_ratios():
    """printed after the margin tests of this module ran (pytest -s shows it); nothing to hold when run on its own"""
    print()
    for k, v in sorted(W.items()):
        print(f"emulation / bound  {k:28s} {v:.3f}")
    for k, v in KAPPA_SEEN.items():
        print(f"kappa reached      {k:28s} {v:.3g}")
    assert all(v < MARGIN for v in W.values())
    if "offset" in KAPPA_SEEN:
        assert KAPPA_SEEN["offset"] >= 100


# ------------------------------------------------------------------------------------------------------------ mutations
def reject_all(muts, ref, tag):
    for label, k, m in muts:
        assert cr.rejected(m, *ref[k]), f"{tag}: mutation '{label}' of {k} accepted"
    return [label for label, _, _ in muts]


def test_forward_mutations_are_rejected_on_the_emulation():
    seen = collections.Counter()
    # the smallest shapes where each applies: one row, a wave, one past a 256 tile, one past a 512 tile; both statistics forms
    for C, L_out, pad in ((16, 1, 0), (64, 1, 2), (48, 17, 2), (16, 17, 20), (64, 257, 2), (16, 257, 2), (48, 513, 2), (64, 513, 20)):
        form = cr.stats_form(3, 1, C, L_out)
        for j, kind in enumerate(cr.KINDS):
            case = cr.make_case(kind, 3, 1, L_out, C, 800 + j, pad=pad)
            emu, ref = fwd_emulated(case, form)
            got = {k: t(v) for k, v in emu.items()}
            for k in ("act", "mean", "rstd", "yx", "x1"):
                cr.check(got[k], *ref[k], what=f"{kind} C={C} L_out={L_out} {k}")
            muts = cr.fwd_mutations(ref, got, case["gamma"], case["beta"], case["eps"], case["geometry"], kind)
            seen.update(reject_all(muts, ref, f"{kind} C={C} L_out={L_out}"))
    for label in ("unbiased variance", "eps left out", "last time step missing from the statistics", "statistics of clip n + 1",
                  "row L_out - 1 zeroed", "first row of the second 256 tile taken from the tile before",
                  "first row of the second 512 tile taken from the tile before"):
        assert seen[label] > 0, label
    assert any(k.startswith("padding row") for k in seen) and any(k.startswith("4-channel group") for k in seen)


def test_backward_mutations_are_rejected_on_the_emulation():
    seen = collections.Counter()
    dense = [(1, 1, 16, 1, "randn"), (9, 1, 16, 17, "randn"), (9, 2, 64, 17, "offset"), (2, 1, 16, 257, "randn"), (2, 1, 64, 257, "tails")]
    for N, C_in, C, L_out, kind in dense:
        case = cr.make_case(kind, N, C_in, L_out, C, 900)
        emu, _ = fwd_emulated(case, cr.stats_form(N, C_in, C, L_out))
        for init in (False, True):
            got, ref = bwd_emulated(case, emu, None, init, 910)
            g = {k: t(v) for k, v in got.items()}
            for k in g:
                cr.check(g[k], *ref[k], what=f"dense {kind} N={N} L_out={L_out} {k}")
            seen.update(reject_all(cr.bwd_mutations(ref, g), ref, f"dense {kind} N={N} C={C} L_out={L_out} init={init}"))
    for counts in ([0, 1, 3], [257, 0]):
        N, L_out = len(counts), 300
        case = cr.make_case("randn", N, 1, L_out, 16, 920)
        emu, _ = fwd_emulated(case, cr.stats_form(N, 1, 16, L_out))
        lists = cr.make_lists(counts, L_out, 921)
        got, ref = bwd_emulated(case, emu, lists, True, 922)
        g = {k: t(v) for k, v in got.items()}
        for k in g:
            cr.check(g[k], *ref[k], what=f"listed {counts} {k}")
        seen.update(reject_all(cr.bwd_mutations(ref, g), ref, f"listed {counts}"))
    for label in ("gelu' evaluated at xh instead of z", "the A2 term dropped", "1 / P for 1 / L_out", "the factor rstd gamma missing",
                  "clips 8.. dropped", "rows 256.. of a clip dropped", "= for +=", "one unlisted row included"):
        assert seen[label] > 0, label


# ------------------------------------------------------------------------------------------------------------ geometry, arguments
def test_stats_form_chunk_count_equals_the_workspace_query():
    from wavjepa_amd import ops
    n = 0
    for N in (1, 2, 3, 8, 64, 200, 256, 500, 1024, 2000):
        for C_in in (1, 2):
            for C in (16, 32, 48, 64, 80, 512, 576):
                for L_out in (1, 31, 32, 33, 255, 256, 257, 513, 1500, 2100, 2177, 6430, 20000):
                    f = cr.stats_form(N, C_in, C, L_out)
                    assert f["chunks"] == -(-L_out // f["tcs"]) and f["tcs"] % 32 == 0
                    assert ops.workspace_bytes("wj_conv0_gn_gelu_fwd", N=N, C_in=C_in, C=C, k=10, L_out=L_out) == f["ws_bytes"], (N, C_in, C, L_out)
                    n += 1
    assert n == 10 * 2 * 7 * 13
    # the statements of the forms the GPU cases rely on
    assert all(cr.stats_form(N, 1, 16, L)["form"] == "fallback" for N in (1, 3, 256) for L in (1, 257, 6430))
    assert cr.stats_form(3, 1, 32, 255)["form"] == "fallback" and cr.stats_form(3, 1, 32, 257)["form"] == "gram"
    assert cr.stats_form(3, 2, 64, 200)["form"] == "fallback" and cr.stats_form(3, 2, 64, 513)["form"] == "gram"
    assert cr.stats_form(3, 1, 48, 1)["form"] == "gram"


def _rc(fn, struct, **fields):
    a = _abi.STRUCTS[struct]()
    for k, v in fields.items():
        setattr(a, k, v)
    return getattr(_abi.load(), fn)(ctypes.byref(a), None)


def test_argument_errors_are_answered_before_a_launch():
    buf = torch.zeros(64)                                   # never dereferenced: every call below returns before its launch
    p = buf.data_ptr()
    N, C_in, C, k, s, L_out = 2, 1, 64, 10, 5, 20
    L = (L_out - 1) * s + k
    fwd = dict(audio=p, w=p, gamma=p, beta=p, act=p, mean=p, rstd=p, workspace=p, N=N, C_in=C_in, L=L, C=C, k=k, stride=s, L_out=L_out,
               P=L_out + 2, eps=1e-5)
    bwd = dict(audio=p, w=p, gamma=p, beta=p, mean=p, rstd=p, dact=p, yx=p, x1=p, dw=p, dgamma=p, dbeta=p, workspace=p, N=N, C_in=C_in,
               L=L, C=C, k=k, stride=s, L_out=L_out, P=L_out + 2)
    ARG, UNSUPPORTED = -1, -3
    f = lambda **kw: _rc("wj_conv0_gn_gelu_fwd", "wj_conv0_fwd_args", **dict(fwd, **kw))      # noqa: E731
    b = lambda **kw: _rc("wj_conv0_gn_gelu_bwd", "wj_conv0_bwd_args", **dict(bwd, **kw))      # noqa: E731
    assert f(C=72) == ARG and f(C=8) == ARG                     # C % 16 forward
    assert b(C=66) == ARG and b(C=2) == ARG                     # C % 4 backward
    assert f(k=9, L=L) == UNSUPPORTED and f(C_in=3, L=L) == UNSUPPORTED and b(k=12, L=200) == UNSUPPORTED and b(C_in=4) == UNSUPPORTED
    assert f(yx=p) == ARG and f(x1=p) == ARG                    # yx without x1 and the reverse
    assert b(yx=0) == ARG and b(x1=0) == ARG
    assert b(rows=p) == ARG and b(rows=p, row_off=p, max_rows=-1) == ARG
    assert f(L=L - 1) == ARG and f(L_out=L_out + 1, P=L_out + 2) == ARG      # (L_out - 1) stride + k > L
    assert f(P=L_out - 1) == ARG and b(P=L_out - 1) == ARG
    assert f(N=0) == ARG and b(L_out=0) == ARG and f(act=0) == ARG and b(dw=0) == ARG


def test_every_field_of_the_argument_structs_is_handled_or_excluded():
    for name, handled in cr.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        excluded = set(cr.EXCLUDED.get(name, {}))
        assert not (handled & excluded), name
        assert fields - handled - excluded == set(), f"{name}: fields without a reference or an exclusion: {sorted(fields - handled - excluded)}"
        assert (handled | excluded) - fields == set(), f"{name}: listed but not in the header: {sorted((handled | excluded) - fields)}"
    assert set(cr.HANDLED) == {"wj_conv0_fwd_args", "wj_conv0_bwd_args"} and not cr.EXCLUDED
