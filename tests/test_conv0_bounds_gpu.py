"""Conv layer 0 in the default mode (wj_conv0_gn_gelu_fwd / wj_conv0_gn_gelu_bwd) held per element against the fp64 reference and
bounds of tests/conv0_reference.py (GPU only).  The shapes are the tables of that module: the smallest that reach each branch of
csrc/conv0.hip (k = 10, stride = 5).

On every case: every output sits NaN-filled between guard rows and must come back finite and within its bound, the guards untouched;
the workspace is NaN-filled with a NaN tail behind the queried size that must stay NaN; a second launch is bit-identical; the padding
rows and the unlisted rows of dact, the audio samples past the last tap and the other channel of a strided batch are NaN; on the small
shapes every mutation that applies is made on the kernel's own (accepted) output and must be rejected.

With WJ_CONV0_BOUNDS_REPORT=<path> the module writes one line per entry, shape class and input kind: the worst error / bound, and the
amplification kappa of the one-pass variance where it applies.
"""
import collections
import os
import time

import pytest
import torch

from tests import conv0_reference as cr

pytestmark = pytest.mark.gpu

REPORT = collections.OrderedDict()
WS_TAIL = 4096            # NaN floats behind the queried workspace size
FWD_OUT = ("act", "mean", "rstd", "yx", "x1")
BWD_OUT = ("dw", "dgamma", "dbeta")


def note(entry, cls, kind, out, ratio, kappa=None):
    key = (entry, cls, kind)
    row = REPORT.setdefault(key, {"kappa": 0.0})
    row[out] = max(row.get(out, 0.0), ratio)
    if kappa is not None:
        row["kappa"] = max(row["kappa"], kappa)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_CONV0_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  shape class  input kind  worst error / bound per output  [kappa]   (tests/test_conv0_bounds_gpu.py)\n")
            for (entry, cls, kind), row in REPORT.items():
                outs = "  ".join(f"{k} {v:.3f}" for k, v in row.items() if k != "kappa")
                kap = f"  kappa {row['kappa']:.3g}" if row["kappa"] else ""
                f.write(f"{entry:22s} {cls:16s} {kind:9s} {outs}{kap}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


def G(M, D=None, dtype=torch.float32, fill=None):
    return cr.guarded_like(M, D, dtype, dev(), fill)


def workspace(ops, fn, **dims):
    n = ops.workspace_bytes(fn, **dims) // 4
    return torch.full((n + WS_TAIL,), float("nan"), device=dev()), n


def reject_all(muts, ref, tag):
    for label, k, m in muts:
        assert cr.rejected(m, *ref[k]), f"{tag}: mutation '{label}' of {k} accepted"


# ------------------------------------------------------------------------------------------------------------ forward
def device_audio(case):
    """the clips on the device, every sample past the last tap NaN"""
    geo = case["geometry"]
    a = case["audio"].to(dev()).clone()
    a[:, :, (geo["L_out"] - 1) * geo["stride"] + geo["k"]:] = float("nan")
    return a


def launch_fwd(ops, case, audio, N, clip_stride=0):
    """one forward launch into NaN-filled guarded outputs and a NaN-filled workspace; returns the Guarded outputs"""
    geo, C, C_in = case["geometry"], case["C"], case["C_in"]
    Tn = C_in * geo["k"]
    P = geo["P"]
    out = {"act": G(N * P, C, torch.bfloat16), "mean": G(N, C), "rstd": G(N, C), "yx": G(N, C * Tn), "x1": G(N, Tn)}
    ws, n = workspace(ops, "wj_conv0_gn_gelu_fwd", N=N, C_in=C_in, C=C, k=geo["k"], L_out=geo["L_out"])
    ops.conv0_fwd(audio, case["w"].to(dev()), case["gamma"].to(dev()), case["beta"].to(dev()), out["act"].view, out["mean"].view,
                  out["rstd"].view, ws, N=N, C_in=C_in, L=case["L"], C=C, k=geo["k"], stride=geo["stride"], L_out=geo["L_out"], P=P,
                  eps=case["eps"], yx=out["yx"].view, x1=out["x1"].view, audio_clip_stride=clip_stride)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n:]).all()), "the workspace was written past its queried size"
    return out


def run_fwd(ops, case, cls, audio=None, clip_stride=0, N_launch=None, mutate=False, distinct=True):
    """two launches (bit-identical), every output held to its bound; returns ({name: device view}, {name: CPU tensor}, reference).
    N_launch: the launch runs that many clips, the first case["N"] of them distinct (the others are held by the caller)."""
    N = case["N"]
    NL = N_launch or N
    geo, C = case["geometry"], case["C"]
    form = cr.stats_form(NL, case["C_in"], C, geo["L_out"], geo["k"])
    audio = device_audio(case) if audio is None else audio
    a = launch_fwd(ops, case, audio, NL, clip_stride)
    b = launch_fwd(ops, case, audio, NL, clip_stride)
    tag = f"{cls} N={NL} C_in={case['C_in']} C={C} L_out={geo['L_out']} P={geo['P']} {case['kind']} [{form['form']}, {cr.apply_form(C)}]"
    views = {k: a[k].check(f"{tag}: {k}") for k in FWD_OUT}
    for k in FWD_OUT:
        assert torch.equal(views[k].view(torch.int16 if k == "act" else torch.int32), b[k].check(k).view(torch.int16 if k == "act" else torch.int32)), \
            f"{tag}: {k} differs between two launches"
    ref = cr.conv0_fwd(case["audio"], case["w"], case["gamma"], case["beta"], case["eps"], geo, form)
    kappa = float(ref["kappa"][0].max()) if geo["L_out"] > 1 else None
    got = {}
    for k in FWD_OUT:
        rows = N * geo["P"] if k == "act" else N
        got[k] = views[k][:rows].cpu()
        note("wj_conv0_gn_gelu_fwd", cls, case["kind"], k, cr.check(got[k], *ref[k], what=f"{tag}: {k}"), kappa)
    if case["kind"] == "offset" and geo["L_out"] > 1:
        print(f"{tag}: kappa up to {kappa:.3g}")
        assert kappa >= 100, tag
    if mutate:
        reject_all(cr.fwd_mutations(ref, got, case["gamma"], case["beta"], case["eps"], geo, case["kind"], distinct), ref, tag)
    return views, got, ref


def fwd_table(ops, table, cls, idx, mutate):
    N, C_in, C, L_out, pad, tail, kinds = table[idx]
    for j, kind in enumerate(kinds):
        run_fwd(ops, cr.make_case(kind, N, C_in, L_out, C, 100 + 10 * idx + j, tail=tail, pad=pad), cls, mutate=mutate)


@pytest.mark.parametrize("idx", range(len(cr.FWD_EDGES)), ids=[f"C{c[2]}-L{c[3]}-pad{c[4]}-tail{c[5]}" for c in cr.FWD_EDGES])
def test_forward_edges(ops, idx):
    """L_out around one step, a wave, a 256 and a 512 tile; MFMA apply (C = 64), VALU apply with Gram statistics (48), fallback
    statistics (16); P - L_out in {0, 2, 20}; 0, 3 or 7 samples behind the last tap; every input kind"""
    fwd_table(ops, cr.FWD_EDGES, "edges", idx, mutate=True)


@pytest.mark.parametrize("idx", range(len(cr.FWD_TWO_CHANNELS)), ids=[f"C{c[2]}-L{c[3]}" for c in cr.FWD_TWO_CHANNELS])
def test_forward_two_channels(ops, idx):
    """20 taps: C = 64 in the fallback form at one chunk (L_out = 200) and in the Gram form at three (513); C = 80 Gram, C = 32 fallback"""
    fwd_table(ops, cr.FWD_TWO_CHANNELS, "two channels", idx, mutate=True)


@pytest.mark.parametrize("idx", range(len(cr.FWD_WIDE)), ids=[f"C{c[2]}-L{c[3]}" for c in cr.FWD_WIDE])
def test_forward_wide(ops, idx):
    """the cb += 512 channel loops: a second pass of the MFMA apply (576) and of the VALU apply (528); exactly one pass (512)"""
    fwd_table(ops, cr.FWD_WIDE, "wide", idx, mutate=cr.FWD_WIDE[idx][3] < 100)


def test_forward_long(ops):
    """the benchmark's time axis: 26 statistics chunks, 13 apply tiles"""
    fwd_table(ops, cr.FWD_LONG, "long", 0, mutate=False)


@pytest.mark.parametrize("idx", range(len(cr.FWD_LONG_CHUNKS)), ids=[f"Cin{c[2]}-L{c[4]}" for c in cr.FWD_LONG_CHUNKS])
def test_forward_long_statistics_chunks(ops, idx):
    """N = 1024 (8 distinct clips repeated): one 2112-step statistics chunk (mono), the 1088-step LDS cap (two channels).  The 8 distinct
    clips are held per element; every other clip must equal its first copy bit for bit, so no element is left out."""
    N, distinct, C_in, C, L_out = cr.FWD_LONG_CHUNKS[idx]
    for j, kind in enumerate(("randn", "offset")):
        case = cr.make_case(kind, distinct, C_in, L_out, C, 300 + j)
        P = case["geometry"]["P"]
        audio = device_audio(case).repeat(N // distinct, 1, 1)
        views, _, _ = run_fwd(ops, case, "long chunks", audio=audio, N_launch=N, distinct=True)
        for k in FWD_OUT:
            v = views[k].view(torch.int16 if k == "act" else torch.int32).reshape(N // distinct, -1)
            assert torch.equal(v, v[:1].expand_as(v)), f"long chunks {kind}: {k} of a repeated clip differs from its first copy"


@pytest.mark.parametrize("N,C,L_out", cr.STRIDED)
def test_forward_strided_audio(ops, N, C, L_out):
    """one channel of an [N][2][L] batch as a mono call (audio = base + c L, audio_clip_stride = 2 L); the other channel is NaN"""
    both = cr.make_case("randn", N, 2, L_out, C, 350, tail=3)
    used = (L_out - 1) * 5 + 10
    for c in range(2):
        case = dict(both, audio=both["audio"][:, c:c + 1].contiguous(), C_in=1, w=both["w"][:, c:c + 1].contiguous())
        batch = torch.full((N, 2, both["L"]), float("nan"), dtype=torch.bfloat16, device=dev())
        batch[:, c, :used] = both["audio"][:, c, :used].to(dev())
        run_fwd(ops, case, "strided", audio=batch[:, c], clip_stride=2 * both["L"], mutate=True)


# ------------------------------------------------------------------------------------------------------------ backward
def launch_bwd(ops, case, audio, st, dact, lists, max_rows, inits):
    geo, C, C_in, N = case["geometry"], case["C"], case["C_in"], case["N"]
    Tn = C_in * geo["k"]
    out = {"dw": G(C, Tn, fill=inits[0]), "dgamma": G(C, fill=inits[1]), "dbeta": G(C, fill=inits[2])}
    ws, n = workspace(ops, "wj_conv0_gn_gelu_bwd", N=N, C_in=C_in, C=C, k=geo["k"], L_out=geo["L_out"], max_rows=max_rows)
    kw = {}
    if lists is not None:
        rows, off, _ = cr.row_lists(lists, geo["P"])
        # an empty rows tensor still needs an address (rows != NULL selects the listed form)
        kw = dict(rows=torch.cat([rows, torch.zeros(1, dtype=torch.int32)]).to(dev()), row_off=off.to(dev()), max_rows=max_rows)
    ops.conv0_bwd(audio, case["w"].to(dev()), case["gamma"].to(dev()), case["beta"].to(dev()), st["mean"], st["rstd"], dact, out["dw"].view,
                  out["dgamma"].view, out["dbeta"].view, ws, yx=st["yx"], x1=st["x1"], N=N, C_in=C_in, L=case["L"], C=C, k=geo["k"],
                  stride=geo["stride"], L_out=geo["L_out"], P=geo["P"], **kw)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[n:]).all()), "the workspace was written past its queried size"
    return out


def run_bwd(ops, case, cls, lists=None, extra_rows=0, both_inits=True, seed=500, mutate=False):
    """forward (held), then the backward on ITS stored mean / rstd / yx / x1 into zeroed and into pre-filled accumulators"""
    geo, C, N = case["geometry"], case["C"], case["N"]
    Tn = case["C_in"] * geo["k"]
    audio = device_audio(case)
    views, stored, _ = run_fwd(ops, case, cls)
    st = {k: views[k].contiguous() for k in ("mean", "rstd", "yx", "x1")}
    dact = cr.make_dact(case, seed)
    if lists is not None:
        dact = cr.mask_unlisted(dact, lists, geo["L_out"])
    max_rows = 0 if lists is None else max(len(tl) for tl in lists) + extra_rows
    g = torch.Generator().manual_seed(seed + 1)
    filled = [torch.randn(C, Tn, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)]
    tag0 = f"{cls} N={N} C_in={case['C_in']} C={C} L_out={geo['L_out']} {case['kind']}" + \
        ("" if lists is None else f" counts={[len(tl) for tl in lists]} max_rows={max_rows}")
    ref0 = None
    for inits in ([None] * 3, filled) if both_inits else (filled,):
        tag = tag0 + (" into zeros" if inits[0] is None else " into randn")
        dev_inits = [torch.zeros_like(f) if i is None else i for i, f in zip(inits, filled)]
        a = launch_bwd(ops, case, audio, st, dact.to(dev()), lists, max_rows, dev_inits)
        b = launch_bwd(ops, case, audio, st, dact.to(dev()), lists, max_rows, dev_inits)
        ref = cr.conv0_bwd(case["audio"], case["w"], case["gamma"], case["beta"], stored["mean"], stored["rstd"], stored["yx"], stored["x1"],
                           dact, geo, lists, *inits, reuse=ref0)
        ref0 = ref
        got = {}
        for k in BWD_OUT:
            got[k] = a[k].check(f"{tag}: {k}").cpu()
            assert torch.equal(got[k].view(torch.int32), b[k].check(k).cpu().view(torch.int32)), f"{tag}: {k} differs between two launches"
            note("wj_conv0_gn_gelu_bwd", cls, case["kind"], k, cr.check(got[k], *ref[k], what=f"{tag}: {k}"))
        if mutate:
            reject_all(cr.bwd_mutations(ref, got, case["kind"]), ref, tag)


@pytest.mark.parametrize("idx", range(len(cr.BWD_DENSE)), ids=[f"N{c[0]}-Cin{c[1]}-C{c[2]}-L{c[3]}" for c in cr.BWD_DENSE])
def test_backward_dense(ops, idx):
    """the 8 clip lanes of the finalize (N = 1, 8, 9, 17), one, two and three 256-row chunks, a partial one, C = 16 / 64 / 576 (a second
    cb += 512 pass), both tap counts; zeroed and pre-filled accumulators"""
    N, C_in, C, L_out, kinds = cr.BWD_DENSE[idx]
    for j, kind in enumerate(kinds):
        run_bwd(ops, cr.make_case(kind, N, C_in, L_out, C, 400 + 10 * idx + j), "dense", seed=500 + idx, mutate=N * L_out * C <= 1 << 20)


@pytest.mark.parametrize("idx", range(len(cr.BWD_LISTED)), ids=[f"{i}-{len(c[0])}clips-extra{c[1]}" for i, c in enumerate(cr.BWD_LISTED)])
def test_backward_listed_rows(ops, idx):
    """clips with zero, one, 255, 256, 257, 513, 600 and all 700 listed rows: clips with different chunk counts (the cnt_off branch of the
    fold, unwritten partial records behind it), max_rows equal to the longest list and larger; the unlisted rows of dact are NaN"""
    counts, extra, kinds = cr.BWD_LISTED[idx]
    lists = cr.make_lists(counts, cr.BWD_LISTED_L_OUT, 600 + idx)
    for j, kind in enumerate(kinds):
        case = cr.make_case(kind, len(counts), 1, cr.BWD_LISTED_L_OUT, 64, 610 + 10 * idx + j)
        run_bwd(ops, case, "listed", lists=lists, extra_rows=extra, both_inits=False, seed=700 + idx, mutate=len(counts) <= 4)
