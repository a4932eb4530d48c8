"""Every attention call of the benchmarked training step, and every branch of the two dispatch tables, replayed against an fp64 reference
with a bound per element (tests/attention_reference.py).

Census: for each workload of bench.WORKLOADS one training step runs through StepRunner at the benchmark's clips per GPU (the GEMM
census's step, tests/test_gemm_census_gpu.py), with ops.attn_fwd / ops.attn_bwd wrapped to record the fields of every call, its seq_off
list or key mask copied to the host.  The calls are deduplicated on their full signature, the model is freed, and every class is
replayed in the flat, peaked, offset and planted regimes: forward into NaN-filled guard-banded outputs, backward fed the kernel's own
out and lse, with defer_fold 1 and 0 (both dbias within the bound of the reference), two launches bit-identical in out / lse / dqkv,
and, in the flat regime, every applicable mutation rejected at the class's own shape.
Dispatch sweep: BRANCHES lists every kernel instantiation wj_attn_fwd / wj_attn_bwd can launch with the T boundaries it owns; each
is run dense, key-masked (mask_group 1 with a fully masked sequence, and 3) and ragged (an empty, a one-token and a full-length
sequence, lengths at 16 k +- 1) in the flat and planted regimes.  The table is held against the launches in attention.hip, so a new
branch without a case fails by name.  A key mask can only mask a key for every query of its sequence, so a single fully masked query
row does not exist in this interface; the fully masked sequence covers the promise (out 0, lse +inf, no gradient).
Key-masked cases with mask_group 1 are also replayed in the ragged form on the packed visible rows (dout zero on the masked rows, which
the ragged form never computes): both within bound of the same fp64 reference.
The extreme regime (the exp overflow probe of attention_reference) runs once per backward kernel family.
WJ_ATTN_CENSUS_REPORT=<path>: the report is also appended there (profiles/attention_census.txt)."""
import gc
import math
import os
import re
import time

import numpy as np
import pytest
import torch

from tests import attention_reference as ar
from tests.test_gemm_census_gpu import CLIPS, _d2h_int32, census as run_census_step, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CENSUS_REGIMES = ("flat", "peaked", "offset", "planted")
SWEEP_REGIMES = ("flat", "planted")


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def _report(lines):
    print("\n".join(lines), flush=True)
    path = os.environ.get("WJ_ATTN_CENSUS_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


# ------------------------------------------------------------------------------------------------------------ dispatch
def fwd_instantiation(f) -> str:
    """the kernel wj_attn_fwd launches (the if-chain at the end of wj_attn_fwd, wavjepa_amd/csrc/attention.hip)"""
    T, hd = f["T"], f["hd"]
    if hd == 16:
        return "attn_fwd_kernel<32, NWF_SHORT, 8, 16>" if T <= 128 else ("attn_fwd_kernel<32, NWF_SHORT, 12, 16>" if T <= 192
                                                                         else "attn_fwd_kernel<32, NWF_LONG, 14, 16>")
    if T > 224:
        return f"attn_fwd_kernel<{hd}, NWF_LONG, 26>"
    if hd == 64:
        return "attn_fwd_kernel<64, NWF_SHORT, 8>" if T <= 128 else "attn_fwd_kernel<64, NWF_LONG, 14>"
    return "attn_fwd_kernel<32, NWF_SHORT, 8>" if T <= 128 else ("attn_fwd_kernel<32, NWF_SHORT, 12>" if T <= 192
                                                                 else "attn_fwd_kernel<32, NWF_LONG, 14>")


def bwd_instantiation(f) -> str:
    """the kernel wj_attn_bwd launches in the release library (the if-chain of launch_bwd, spelled as there without its last argument DET;
    WJ_ATTN_BWD_FRAG is a laboratory switch)"""
    T, hd = f["T"], f["hd"]
    m = "true" if f["form"] == "mask" else "false"
    if hd == 16:
        if T <= 128:
            return f"attn_bwd_frag_kernel<32, NWB32, 8, {m}, 16>"
        return f"attn_bwd_frag_kernel<32, NWB32, 12, {m}, 16>" if T <= 192 else "attn_bwd_kernel<32, NWB32, 14, 16>"
    if T > 224:
        return f"attn_bwd_kernel<{hd}, NWB{hd}, 26, {hd}>"
    if T <= 128:
        return f"attn_bwd_frag_kernel<{hd}, NWB{hd}, 8, {m}, {hd}>"
    if hd == 64:
        return "attn_bwd_kernel<64, NWB64, 14, 64>"
    return f"attn_bwd_frag_kernel<32, NWB32, 12, {m}, 32>" if T <= 192 else "attn_bwd_kernel<32, NWB32, 14, 32>"


BOUNDARIES = (1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 191, 192, 193, 223, 224, 225, 415, 416)
# instantiation: (head width, first T, last T) -- every launch of the two dispatch tables; the cases of the sweep are generated from it
BRANCHES = {
    "attn_fwd_kernel<32, NWF_SHORT, 8, 16>": (16, 1, 128), "attn_fwd_kernel<32, NWF_SHORT, 12, 16>": (16, 129, 192),
    "attn_fwd_kernel<32, NWF_LONG, 14, 16>": (16, 193, 224),
    "attn_fwd_kernel<64, NWF_LONG, 26>": (64, 225, 416), "attn_fwd_kernel<32, NWF_LONG, 26>": (32, 225, 416),
    "attn_fwd_kernel<64, NWF_SHORT, 8>": (64, 1, 128), "attn_fwd_kernel<64, NWF_LONG, 14>": (64, 129, 224),
    "attn_fwd_kernel<32, NWF_SHORT, 8>": (32, 1, 128), "attn_fwd_kernel<32, NWF_SHORT, 12>": (32, 129, 192),
    "attn_fwd_kernel<32, NWF_LONG, 14>": (32, 193, 224),
    "attn_bwd_frag_kernel<32, NWB32, 8, true, 16>": (16, 1, 128), "attn_bwd_frag_kernel<32, NWB32, 8, false, 16>": (16, 1, 128),
    "attn_bwd_frag_kernel<32, NWB32, 12, true, 16>": (16, 129, 192), "attn_bwd_frag_kernel<32, NWB32, 12, false, 16>": (16, 129, 192),
    "attn_bwd_kernel<32, NWB32, 14, 16>": (16, 193, 224),
    "attn_bwd_kernel<64, NWB64, 26, 64>": (64, 225, 416), "attn_bwd_kernel<32, NWB32, 26, 32>": (32, 225, 416),
    "attn_bwd_frag_kernel<64, NWB64, 8, true, 64>": (64, 1, 128), "attn_bwd_frag_kernel<64, NWB64, 8, false, 64>": (64, 1, 128),
    "attn_bwd_frag_kernel<32, NWB32, 8, true, 32>": (32, 1, 128), "attn_bwd_frag_kernel<32, NWB32, 8, false, 32>": (32, 1, 128),
    "attn_bwd_kernel<64, NWB64, 14, 64>": (64, 129, 224),
    "attn_bwd_frag_kernel<32, NWB32, 12, true, 32>": (32, 129, 192), "attn_bwd_frag_kernel<32, NWB32, 12, false, 32>": (32, 129, 192),
    "attn_bwd_kernel<32, NWB32, 14, 32>": (32, 193, 224),
}
# reached only with WJ_ATTN_BWD_FRAG = 0 in the laboratory library (the suite loads the release one); their code is the general kernel's,
# which the T > 128 cases run at 14 and 26 tiles
LAB_ONLY = {"attn_bwd_kernel<64, NWB64, 8, 64>", "attn_bwd_kernel<32, NWB32, 8, 32>"}


def test_branch_table_lists_every_launch_of_the_source():
    src = open(os.path.join(ROOT, "wavjepa_amd", "csrc", "attention.hip")).read()
    # launch_bwd is one chain for the default and the deterministic instantiations: every backward launch ends in `, DET>`
    launched = set(m + ">" for m in re.findall(r"hipLaunchKernelGGL\(\((attn_\w+<[^>]*?)(?:, DET)?>\)", src))
    assert len(re.findall(r"hipLaunchKernelGGL\(\(attn_bwd\w+<[^>]*, DET>\)", src)) == len(re.findall(r"hipLaunchKernelGGL\(\(attn_bwd", src)) == 17
    assert len(launched) == 27, sorted(launched)
    missing = launched - set(BRANCHES) - LAB_ONLY
    assert not missing, f"launches of attention.hip without a branch (and so without a case) in the sweep: {sorted(missing)}"
    assert not set(BRANCHES) - launched, f"branches the source no longer launches: {sorted(set(BRANCHES) - launched)}"


# ------------------------------------------------------------------------------------------------------------ replay
def _launch_fwd(ops, o):
    ops.attn_fwd(**o.fwd_kwargs())
    torch.cuda.synchronize()


def _launch_bwd(ops, o, defer):
    ops.attn_bwd(**o.bwd_kwargs(defer))
    torch.cuda.synchronize()


def _bits_equal(o, names, a, b):
    return [n for n in names if not torch.equal(ar._ibits(a[n]), ar._ibits(b[n]))]


def replay(ops, f, regime, fails, backward=True, mutate=False, seed=0, zero_dout_on_masked=False):
    """one class in one regime; returns (operands, forward reference, backward reference, worst err / bound per output)"""
    o = ar.Operands(f, dev(), seed=seed, regime=regime)
    if zero_dout_on_masked:
        mk = torch.zeros(o.R, dtype=torch.bool, device=dev())
        mk[o.ix.row[o.ix.qval & ~o.ix.kval]] = True
        o.view("dout")[mk] = 0
    per = {}
    snap_f = o.snapshot("fwd")
    _launch_fwd(ops, o)
    ex_f = ar.reference_fwd(o)
    bad, _ = ar.check(o, ex_f, snap_f, "fwd")
    per.update(ar.LAST)
    fails += [f"{regime} forward: {b}" for b in bad]
    outs_f = {n: o.b[n].t.clone() for n in snap_f}
    o.reset_outputs("fwd")
    _launch_fwd(ops, o)
    diff = _bits_equal(o, snap_f, outs_f, {n: o.b[n].t for n in snap_f})
    if diff:
        fails.append(f"{regime} forward: two launches differ in {diff}")
    ex_b, outs_b = None, None
    if backward:
        assert f["lse"]
        kept = {}
        snap_b = o.snapshot("bwd")
        for defer in (f["defer_fold"], not f["defer_fold"]):
            o.reset_outputs("bwd")
            _launch_bwd(ops, o, defer)
            if ex_b is None:
                ex_b = ar.reference_bwd(o, ex_f)
            bad, _ = ar.check(o, ex_b, snap_b, "bwd", folded=not defer)
            for k, v in ar.LAST.items():
                per[k] = max(per.get(k, 0.0), v)
            fails += [f"{regime} backward defer_fold={int(defer)}: {b}" for b in bad]
            kept[defer] = {n: o.b[n].t.clone() for n in snap_b}
        if not torch.equal(ar._ibits(kept[True]["dqkv"]), ar._ibits(kept[False]["dqkv"])):
            fails.append(f"{regime} backward: dqkv differs between defer_fold 1 and 0")
        o.reset_outputs("bwd")
        _launch_bwd(ops, o, False)
        if not torch.equal(ar._ibits(o.b["dqkv"].t), ar._ibits(kept[False]["dqkv"])):
            fails.append(f"{regime} backward: two launches differ in dqkv")
        outs_b = kept[False]
    if mutate:
        n = 0
        for what, phase, mutated in ar.mutations(o, outs_f, outs_b, folded=True):
            n += 1
            if not ar.check(o, ex_f if phase == "fwd" else ex_b, snap_f if phase == "fwd" else snap_b, phase, mutated, folded=True)[0]:
                fails.append(f"{regime}: mutation '{what}' was not rejected")
        if n < (8 if backward else 4):
            fails.append(f"{regime}: only {n} mutations applied")
    return o, ex_f, ex_b, per


def replay_ragged_twin(ops, f, fails, seed=0):
    """a key-masked class (mask_group 1) in the ragged form on its packed visible rows, against the dense form's reference"""
    fl = []
    o, ex_f, ex_b, per = replay(ops, f, "flat", fl, seed=seed, zero_dout_on_masked=True)
    fails += [f"dense form with dout zero on masked rows: {x}" for x in fl]
    vis = ~torch.as_tensor(f["mask"])
    lens = vis.sum(1).numpy()
    if int(lens.max()) == 0:
        return per
    g = ar.fields(f["B"], int(lens.max()), f["H"], f["hd"], "ragged", seq_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32),
                  lse=f["lse"], dbias=f["dbias"], defer_fold=f["defer_fold"])
    o2 = ar.Operands(g, dev(), seed=seed)
    rows = torch.nonzero(vis.reshape(-1)).flatten().to(dev())
    o2.view("qkv")[:] = o.view("qkv")[rows]
    o2.view("dout")[:] = o.view("dout")[rows]
    snap_f, snap_b = o2.snapshot("fwd"), o2.snapshot("bwd")
    _launch_fwd(ops, o2)
    e2f = ar.reference_fwd(o2)
    bad, _ = ar.check(o2, e2f, snap_f, "fwd")
    fails += [f"ragged twin fwd: {x}" for x in bad]
    worst = dict(ar.LAST)
    # the backward's reference depends on the bf16 out and the lse it is given: hand the ragged backward the dense forward's (both
    # forwards are inside the same bound), so that the two backward references are one
    o2.view("out")[:] = o.view("out")[rows]
    o2.set_lse_rows(o.lse_rows()[rows], o2.b["lse"].t)
    _launch_bwd(ops, o2, g["defer_fold"])
    e2b = ar.reference_bwd(o2, e2f)
    bad, _ = ar.check(o2, e2b, snap_b, "bwd")
    fails += [f"ragged twin bwd: {x}" for x in bad]
    worst.update(ar.LAST)
    for k, v in worst.items():
        per[k] = max(per.get(k, 0.0), v)
    for name, a, b in (("out", e2f.ref["out"], ex_f.ref["out"][rows]), ("lse", e2f.ref["lse"], ex_f.ref["lse"][rows]),
                       ("dqkv", e2b.ref["dqkv"], ex_b.ref["dqkv"][rows])):
        if not bool(((a - b).abs() <= 1e-9 * (1 + b.abs())).all()):
            fails.append(f"ragged twin: the two forms' fp64 references differ in {name} (by {float((a - b).abs().max()):.3g})")
    return per


def _fmt(per):
    return " ".join(f"{k}={v:.3f}" for k, v in per.items())


# ------------------------------------------------------------------------------------------------------------ census
def _host_mask(km, n):
    if isinstance(km, torch.Tensor):
        torch.cuda.synchronize()
        return km.reshape(-1)[:n].cpu().numpy().astype(bool)
    assert n % 4 == 0, n
    return _d2h_int32(km, n // 4).view(np.uint8).astype(bool)


def _fields_of(kind, kw):
    B, T, H, hd = kw["B"], kw["T"], kw["H"], kw["hd"]
    g = kw.get("mask_group", 1)
    form, mask, off = "none", None, None
    if kw.get("seq_off") is not None:
        form, off = "ragged", _d2h_int32(kw["seq_off"], B + 1)
    elif kw.get("key_mask") is not None:
        rows = (B + g - 1) // g
        form, mask = "mask", _host_mask(kw["key_mask"], rows * T).reshape(rows, T)
    if kind == "fwd":
        return ar.fields(B, T, H, hd, form, mask, off, g, lse=kw.get("lse") is not None, dbias=False)
    return ar.fields(B, T, H, hd, form, mask, off, g, lse=True, dbias=kw.get("dbias") is not None, defer_fold=bool(kw.get("defer_fold", False)))


def attention_census(ops, monkeypatch, workload, clips):
    calls = []
    real_f, real_b = ops.attn_fwd, ops.attn_bwd

    def attn_fwd(qkv, out, **kw):
        calls.append(("fwd", _fields_of("fwd", kw)))
        return real_f(qkv, out, **kw)

    def attn_bwd(qkv, out, dout, lse, dqkv, **kw):
        calls.append(("bwd", _fields_of("bwd", kw)))
        return real_b(qkv, out, dout, lse, dqkv, **kw)

    with monkeypatch.context() as mp:
        mp.setattr(ops, "attn_fwd", attn_fwd)
        mp.setattr(ops, "attn_bwd", attn_bwd)
        run_census_step(ops, monkeypatch, workload, clips)         # builds the model, runs one step, frees it
    seen = {}
    for kind, f in calls:
        key = (kind, ar.signature(f))
        if key not in seen:
            seen[key] = [kind, f, 0]
        seen[key][2] += 1
    return calls, list(seen.values())


@pytest.mark.parametrize("workload", sorted(CLIPS))
def test_attention_census_replays_within_the_fp64_bound(ops, monkeypatch, workload):
    t0 = time.perf_counter()
    clips = CLIPS[workload]
    calls, cls = attention_census(ops, monkeypatch, workload, clips)
    t_census = time.perf_counter() - t0
    fs = [f for _, f, _ in cls]
    assert any(f["form"] == "none" for f in fs), "no dense unmasked class (the teacher) in the census"
    assert {f["hd"] for f in fs if f["form"] == "ragged"} >= {32, 64}, "ragged classes for both head widths expected"
    assert any(k == "bwd" and f["defer_fold"] for k, f, _ in cls), "no backward with defer_fold = 1 in the census"
    failing, lines = [], []
    for i, (kind, f, count) in enumerate(cls):
        fails, ran, worst = [], [], {}
        for regime in CENSUS_REGIMES:
            _, _, _, per = replay(ops, f, regime, fails, backward=kind == "bwd", mutate=regime == "flat", seed=100 + i)
            ran.append(regime)
            worst[regime] = max(per.values())
            gc.collect()
            torch.cuda.empty_cache()
        if f["form"] == "mask" and f["mask_group"] == 1 and kind == "bwd":
            replay_ragged_twin(ops, f, fails, seed=100 + i)
            ran.append("ragged twin")
        inst = fwd_instantiation(f) if kind == "fwd" else fwd_instantiation(f) + " + " + bwd_instantiation(f)
        line = (f"{workload} x{count} {kind} {ar.describe(f)} | {inst} | ran {','.join(ran)} (fwd x2" + (", bwd defer_fold 1/0 + repeat"
                if kind == "bwd" else "") + ", mutations in flat) | max err/bound " + " ".join(f"{r}={w:.3f}" for r, w in worst.items())
                + (" | FAIL" if fails else ""))
        lines.append(line)
        print(line, flush=True)
        if fails:
            failing.append(line + "\n    " + "\n    ".join(fails[:10]))
    elapsed = time.perf_counter() - t0
    summary = f"{workload}: {clips} clips per GPU, {len(calls)} attention calls, {len(cls)} classes; census {t_census:.1f} s, total {elapsed:.1f} s"
    _report([summary] + lines)
    assert not failing, f"{len(failing)} of {len(cls)} classes failed:\n" + "\n".join(failing)


# ------------------------------------------------------------------------------------------------------------ dispatch sweep
def _sweep_mask(rows, T, seed, full_row=None):
    g = np.random.default_rng(seed)
    m = g.random((rows, T)) < 0.6
    m[:, T // 2] = False
    if full_row is not None:
        m[full_row] = True
    return m


def _sweep_lengths(T):
    k = (T - 1) // 16
    return [0, 1, T, min(T, max(1, 16 * k - 1)), min(T, 16 * k + 1), max(1, T // 2)]


def sweep_cases():
    """(name, fields) of every (head width, boundary T, form) the branch table owns, plus the large-grid case"""
    cases = []
    combos = sorted({(hd, T) for hd, lo, hi in BRANCHES.values() for T in BOUNDARIES if lo <= T <= hi})
    for hd, T in combos:
        H = 3                                                                       # B x H = 9 or 18: not a multiple of the 8 XCDs
        cases.append((f"hd{hd} T{T} none", ar.fields(3, T, H, hd)))
        cases.append((f"hd{hd} T{T} mask", ar.fields(3, T, H, hd, "mask", mask=_sweep_mask(3, T, T, full_row=1))))
        cases.append((f"hd{hd} T{T} mask/3", ar.fields(6, T, H, hd, "mask", mask=_sweep_mask(2, T, T + 1), mask_group=3)))
        cases.append((f"hd{hd} T{T} ragged", ar.fields(6, T, H, hd, "ragged", seq_off=np.concatenate([[0], np.cumsum(_sweep_lengths(T))]),
                                                       defer_fold=T % 2 == 1)))
    cases.append(("hd32 T40 mask, 2160 workgroups", ar.fields(180, 40, 12, 32, "mask", mask=_sweep_mask(180, 40, 7))))
    return cases


def test_dispatch_sweep(ops):
    t0 = time.perf_counter()
    cases = sweep_cases()
    covered, failing, lines = {}, [], []
    for i, (name, f) in enumerate(cases):
        fails, worst = [], {}
        for regime in SWEEP_REGIMES:
            _, _, _, per = replay(ops, f, regime, fails, seed=500 + i)
            worst[regime] = max(per.values())
        ran = list(SWEEP_REGIMES)
        if f["form"] == "mask" and f["mask_group"] == 1:
            replay_ragged_twin(ops, f, fails, seed=500 + i)
            ran.append("ragged twin")
        insts = (fwd_instantiation(f), bwd_instantiation(f))
        for inst in insts:
            assert inst in BRANCHES, f"{name}: dispatches to {inst}, which the branch table does not list"
            covered.setdefault(inst, set()).add((f["T"], f["form"], f["mask_group"]))
        line = (f"sweep {name} B={f['B']} H={f['H']} | {insts[0]} + {insts[1]} | ran {','.join(ran)} | max err/bound "
                + " ".join(f"{r}={w:.3f}" for r, w in worst.items()) + (" | FAIL" if fails else ""))
        lines.append(line)
        if fails:
            failing.append(line + "\n    " + "\n    ".join(fails[:10]))
    for inst, (hd, lo, hi) in BRANCHES.items():
        got = covered.get(inst, set())
        assert got, f"branch {inst} of the dispatch tables has no case"
        forms = [("none", 1), ("ragged", 1)] if ", false" in inst else [("mask", 1), ("mask", 3)] if ", true" in inst else \
            [("none", 1), ("ragged", 1), ("mask", 1), ("mask", 3)]
        for T in (t for t in BOUNDARIES if lo <= t <= hi):
            for form, g in forms:
                assert (T, form, g) in got, f"branch {inst} has no case at T = {T}, {form}, mask_group {g}"
    summary = f"dispatch sweep: {len(cases)} cases x {len(SWEEP_REGIMES)} regimes over {len(BRANCHES)} instantiations, {time.perf_counter() - t0:.1f} s"
    _report([summary] + lines)
    assert not failing, f"{len(failing)} of {len(cases)} cases failed:\n" + "\n".join(failing)


# ------------------------------------------------------------------------------------------------------------ extreme regime
EXTREME_CASES = {
    "general": ar.fields(4, 150, 2, 64, "mask", mask=_sweep_mask(4, 150, 11)),
    "frag masked": ar.fields(4, 39, 2, 32, "mask", mask=_sweep_mask(4, 39, 12)),
    "frag unmasked": ar.fields(4, 40, 2, 32, "ragged", seq_off=np.concatenate([[0], np.cumsum([40, 39, 33, 23])])),
    "frag unmasked hd64": ar.fields(4, 40, 2, 64, "ragged", seq_off=np.concatenate([[0], np.cumsum([40, 39, 33, 23])])),
}


@pytest.mark.parametrize("family", sorted(EXTREME_CASES))
def test_extreme_scores_give_no_nan(ops, family):
    """A masked key whose scaled score exceeds its row's lse by more than 90, and a row with lse < -90 in front of padding keys
    (T % 16 != 0): exp(s - lse) of that key overflows fp32, and the backward must still return the reference's finite gradient.
    The magnitudes this takes (all hd elements of the query row and of the key rows at +-a): a = 3.5 at hd 64, 4.25 at hd 32, 5.0 at
    hd 16 -- far inside bf16, large for projections of LayerNorm outputs (|q| = |k| = 28 at hd 64).  With the mask applied as a product
    behind the exp (the kernels before this test) the masked-key case returned NaN in 512 dqkv elements of the frag kernel at
    B = 4, T = 39; the mask now sits inside the exponent (attention.hip, the note in front of attn_bwd_kernel)."""
    f = EXTREME_CASES[family]
    fails = []
    o, _, _, per = replay(ops, f, "extreme", fails)
    _report([f"extreme {family} {ar.describe(f)} | {fwd_instantiation(f)} + {bwd_instantiation(f)} | magnitude {o.extreme_scale} | "
             f"max err/bound {_fmt(per)}" + (" | FAIL" if fails else "")])
    assert not fails, "\n".join(fails[:10])
