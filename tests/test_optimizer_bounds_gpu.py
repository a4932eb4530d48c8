"""The optimiser pass (wj_grad_sumsq, wj_adamw_step, wj_ema_update, wj_cast_f32_to_bf16) held per element against the fp64 references
and bounds of tests/optimizer_reference.py (GPU only).

Every launch runs on a sub-range [lo, lo + n) of a larger flat buffer, as FusedAdamW.step calls it (p32 + 4 lo, p16 + 2 lo): lo = 4
and 12 floats leave the bf16 shadow pointer 8-byte aligned only.  Everything outside the range is NaN before the launch and must be
NaN after it; every element inside must come back finite and within its bound.  Sizes: one lane, the last lane of a workgroup, the
first lane of a second one, a large odd count; `workgroups` 0, 1 and 3 (the stride loop at small n); one EMA and one sumsq case above
their grid caps.  At n = 1028 every mutation the reference claims is made on the kernel's own (accepted) output and must be rejected,
and every REQUIRED one must be claimed.

With WJ_OPT_BOUNDS_REPORT=<path> the module writes one line per entry, size, kind and state with the worst error / bound, and its
wall time.
"""
import collections
import ctypes
import os
import time

import pytest
import torch

from tests import norm_reference as nr
from tests import optimizer_reference as orf

pytestmark = pytest.mark.gpu

WJ_ERR_ARG = -1                      # csrc/common.h
N_MUT = 1028
# (n, lo, workgroups)
ADAMW_CASES = [(4, 0, 0), (4, 12, 3), (1020, 4, 1), (1028, 12, 3), (1028, 0, 0), (1028, 4, 1), (4 * 100003, 4, 0), (4 * 100003, 12, 3)]
SUMSQ_BIG = 4 * (1024 * 256 + 77)
EMA_BIG = 4 * (8192 * 256 + 77)

REPORT = collections.OrderedDict()


def note(entry, n, kind, ratio):
    key = (entry, n, kind)
    REPORT[key] = max(REPORT.get(key, 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_OPT_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  n  kind / state  worst error / bound   (tests/test_optimizer_bounds_gpu.py)\n")
            for (entry, n, kind), ratio in REPORT.items():
                f.write(f"{entry:22s} n={n:<9} {kind:24s} {ratio:.3f}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


class Range:
    """[lo, lo + n) of a flat NaN-filled buffer between guard rows: `inside` is what a launch may touch"""
    def __init__(self, n, lo, dtype=torch.float32, fill=None):
        self.n, self.lo = n, lo
        self.g = nr.guarded_like((lo + n + 3) // 4 + 1, 4, dtype, dev())
        self.flat = self.g.view.reshape(-1)
        self.inside = self.flat[lo:lo + n]
        if fill is not None:
            self.inside.copy_(fill)

    @property
    def ptr(self):
        return self.inside.data_ptr()

    def check(self, what):
        assert self.g.guards_intact(), f"{what}: a guard row was written"
        assert bool(torch.isnan(self.flat[:self.lo].float()).all()) and bool(torch.isnan(self.flat[self.lo + self.n:].float()).all()), \
            f"{what}: an element outside [lo, lo + n) was written"
        return self.inside.cpu()


def held(entry, n, kind, got, pair, what):
    if isinstance(got, Range):
        got = got.check(what)
    ratio = nr.check(got, *pair, what=f"{entry} n={n} {kind} {what}")
    note(entry, n, kind, ratio)
    return got


def run_sumsq(ops, g, n, lo, wg=0, out0=None):
    """one launch on a range; returns the f32 [1] result (CPU) after the guards of out and workspace were checked"""
    gr = Range(n, lo, fill=g)
    out = nr.guarded_like(1, 1, torch.float32, dev(), None if out0 is None else out0.reshape(1, 1))
    ws = nr.guarded_like(1, 1024, torch.float32, dev())
    ops.grad_sumsq(gr.ptr, out.view, ws.view, n, accumulate=out0 is not None, workgroups=wg)
    ws.check("sumsq workspace")
    assert torch.equal(gr.check("sumsq g"), g), "grad_sumsq wrote its input"
    return out.check("sumsq out").cpu().reshape(1)


def run_adamw(ops, c, n, lo, wg, sumsq, zero_grad=False, with_bf16=True):
    """one launch on fresh copies of the case's p, g, m, v; returns {p, m, v, p_bf16, g} on the CPU"""
    r = {k: Range(n, lo, fill=c[k]) for k in ("p", "g", "m", "v")}
    pb = Range(n, lo, torch.bfloat16)
    H = c["H"]
    ops.adamw_step(r["p"].ptr, r["g"].ptr, r["m"].ptr, r["v"].ptr, n, lr=H["lr"], beta1=H["beta1"], beta2=H["beta2"], eps=H["eps"],
                   weight_decay=H["weight_decay"], step=c["step"], max_norm=c.get("max_norm", H["max_norm"]), sumsq=sumsq,
                   p_bf16=pb.ptr if with_bf16 else None, grad_scale=c["grad_scale"], workgroups=wg, zero_grad=zero_grad)
    got = {k: x.check(k) for k, x in r.items()}
    got["p_bf16"] = pb.check("p_bf16")
    return got


# ------------------------------------------------------------------------------------------------------------ AdamW
@pytest.mark.parametrize("n,lo,wg", ADAMW_CASES)
def test_adamw_every_kind_and_state(ops, n, lo, wg):
    big = n > 4096
    for i, kind in enumerate(orf.KINDS):
        for hyper in (("project", "nowd")[i % 2],) if big else tuple(orf.HYPER):
            for state in orf.STATES:
                c = orf.adamw_case(kind, state, n, hyper, 100 + i)
                tag = f"{kind} / {state}"
                Fd = orf.fields(c["H"], c["step"], c["grad_scale"])
                ss = run_sumsq(ops, c["g"], n, lo, wg)
                held("grad_sumsq", n, tag, ss, orf.grad_sumsq(c["g"])["out"], f"{hyper} lo={lo} workgroups={wg}")
                ssd = ss.to(dev())
                ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd)
                got = run_adamw(ops, c, n, lo, wg, ssd)
                for k in ("p", "m", "v", "p_bf16", "g"):
                    held("adamw_step." + k, n, tag, got[k], ref[k], f"{hyper} lo={lo} workgroups={wg}")
                assert torch.equal(got["p_bf16"], got["p"].to(torch.bfloat16)), f"{tag}: p_bf16 is not bf16 of the p the launch wrote"
                again = run_adamw(ops, c, n, lo, wg, ssd)
                for k in got:
                    assert torch.equal(got[k], again[k]), f"{tag}: {k} differs between two launches"
                zg = run_adamw(ops, c, n, lo, wg, ssd, zero_grad=True)
                assert bool((zg["g"] == 0).all()), f"{tag}: zero_grad left a gradient"
                nr.check(zg["g"], *orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd, zero_grad=True)["g"], what="g with zero_grad")
                for k in ("p", "m", "v", "p_bf16"):
                    assert torch.equal(got[k], zg[k]), f"{tag}: {k} with zero_grad differs from the update without it"
                if state == "fresh" and kind == "randn":        # without the shadow: the same update, the shadow left alone
                    nb = run_adamw(ops, c, n, lo, wg, ssd, with_bf16=False)
                    assert bool(torch.isnan(nb["p_bf16"].float()).all()) and all(torch.equal(nb[k], got[k]) for k in ("p", "m", "v"))
                if n == N_MUT:
                    muts = orf.adamw_mutations(c, ss, Fd, got, ref)
                    assert not orf.required_missing(c, muts), orf.required_missing(c, muts)
                    for label, k, m, claimed in muts:
                        if claimed:
                            assert nr.rejected(m, *ref[k]), f"{hyper} {tag}: mutation '{label}' of {k} accepted"


def test_adamw_clipping_switched_off(ops):
    """max_norm <= 0, or no sumsq: the gradient is scaled by grad_scale alone, whatever its norm"""
    n, lo = 1028, 4
    for i, (kind, mx, with_ss) in enumerate((("clipped", 0.0, True), ("clipped", -1.0, True), ("scaled", None, False))):
        c = orf.adamw_case(kind, "warm", n, "project", 130 + i)
        if mx is not None:
            c["max_norm"] = mx
        ss = run_sumsq(ops, c["g"], n, lo)
        Fd = orf.fields(c["H"], c["step"], c["grad_scale"], max_norm=mx)
        ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss if with_ss else None, Fd)
        got = run_adamw(ops, c, n, lo, 0, ss.to(dev()) if with_ss else None)
        for k in ("p", "m", "v", "p_bf16", "g"):
            held("adamw_step." + k, n, f"{kind} / no clip", got[k], ref[k], f"max_norm={mx} sumsq={with_ss}")
        clip = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, orf.fields(c["H"], c["step"], c["grad_scale"]))
        assert nr.rejected(got["m"], *clip["m"]), "the clipped update passes as the unclipped one"


def test_adamw_twenty_chained_steps(ops):
    """The gradient is drawn per step (clip inactive, active, active on the scaled norm in turn); each step's reference starts from the
    kernel's own previous p, m, v, so that the single-step bound holds at every step: a wrong bc1 or bc2 at step k has no drift to
    hide behind."""
    n, lo = 1028, 4
    for hyper in orf.HYPER:
        H = orf.HYPER[hyper]
        c = orf.adamw_case("randn", "fresh", n, hyper, 140)
        for step in range(1, 21):
            kind = ("randn", "clipped", "scaled")[step % 3]
            c["g"], c["grad_scale"] = orf.make_grad(kind, n, 1400 + step, H)
            c["step"] = step
            Fd = orf.fields(H, step, c["grad_scale"])
            ss = run_sumsq(ops, c["g"], n, lo, step % 4)
            ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd)
            got = run_adamw(ops, c, n, lo, step % 4, ss.to(dev()), zero_grad=bool(step % 2))
            for k in ("p", "m", "v", "p_bf16"):
                held("adamw_step." + k, n, f"chained / {hyper}", got[k], ref[k], f"step {step} ({kind})")
            wrong = orf._adamw(*(nr.f64(c[k]) for k in ("p", "g", "m", "v")), ss, orf.fields(H, step + 1, c["grad_scale"]))
            right = orf._adamw(*(nr.f64(c[k]) for k in ("p", "g", "m", "v")), ss, Fd)
            assert nr.rejected(nr.f64(got["p"]) + wrong["p"] - right["p"], *ref["p"]), f"step {step}: the next step's bc1 and bc2 accepted"
            c["p"], c["m"], c["v"] = got["p"], got["m"], got["v"]


# ------------------------------------------------------------------------------------------------------------ sumsq
@pytest.mark.parametrize("n", [4, 1020, 1028, 4 * 100003, SUMSQ_BIG])
def test_grad_sumsq(ops, n):
    g, _ = orf.make_grad("randn", n, 150, orf.HYPER["project"])
    for lo in (0, 4, 12):
        for wg in (0, 1, 3):
            ref = orf.grad_sumsq(g)["out"]
            got = held("grad_sumsq", n, "randn", run_sumsq(ops, g, n, lo, wg), ref, f"lo={lo} workgroups={wg}")
            assert torch.equal(got, run_sumsq(ops, g, n, lo, wg)), "grad_sumsq differs between two launches"
            out0 = (0.5 * ref[0]).float()
            refa = orf.grad_sumsq(g, out0, True)["out"]
            gota = held("grad_sumsq", n, "randn, accumulate", run_sumsq(ops, g, n, lo, wg, out0), refa, f"lo={lo} workgroups={wg}")
            assert nr.rejected(orf.mutate_sumsq_ignore_out0(gota, out0), *refa), "accumulate ignoring out0 accepted"
            if n <= 2 ** 20:
                assert orf.sumsq_last_vector_separates(g)
                assert nr.rejected(orf.mutate_sumsq_drop_last(got, g), *ref), "the last vector dropped accepted"


def test_grad_sumsq_by_sections_feeds_adamw(ops):
    """`accumulate` over the sections of a range with alternating `workgroups`, held against the fp64 sum of the whole (the bound: the
    sections' bounds added, each final add at its running value), then handed to wj_adamw_step as its sumsq"""
    n, lo = 4 * 100003, 4
    c = orf.adamw_case("clipped", "warm", n, "project", 160)
    gr = Range(n, lo, fill=c["g"])
    cuts = [0, 4, 4 * 1000, 4 * 77777, 4 * 77778, n]
    out = nr.guarded_like(1, 1, torch.float32, dev(), torch.full((1, 1), 123.0))     # (overwritten by the first, non-accumulating section)
    ws = nr.guarded_like(1, 1024, torch.float32, dev())
    g64 = nr.f64(c["g"])
    run, bound = 0.0, 0.0
    for k, (a, b) in enumerate(zip(cuts, cuts[1:])):
        ops.grad_sumsq(gr.ptr + 4 * a, out.view, ws.view, b - a, accumulate=k > 0, workgroups=0 if k % 2 else 37)
        s = float((g64[a:b] ** 2).sum())
        run += s
        bound += nr.KAPPA * nr.U * s + (nr.U * run if k > 0 else 0.0)
    ss = out.check("out").cpu().reshape(1)
    ws.check("workspace")
    whole = orf.grad_sumsq(c["g"])["out"][0]
    assert abs(run - float(whole)) < 1e-12 * run
    held("grad_sumsq", n, "by sections", ss, (whole, torch.tensor([bound], dtype=torch.float64)), "five sections")
    Fd = orf.fields(c["H"], c["step"], c["grad_scale"])
    ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd)
    got = run_adamw(ops, c, n, lo, 0, ss.to(dev()))
    for k in ("p", "m", "v", "p_bf16", "g"):
        held("adamw_step." + k, n, "sumsq by sections", got[k], ref[k], "clipped / warm")


# ------------------------------------------------------------------------------------------------------------ EMA
@pytest.mark.parametrize("n,lo", [(4, 0), (4, 12), (1020, 4), (1028, 12), (1028, 0), (4 * 100003, 4), (EMA_BIG, 12)])
def test_ema_update(ops, n, lo):
    s, t = orf.ema_case(n, 170)
    sd = Range(n, lo, fill=s)
    for r in orf.EMA_SCHEDULE if n < EMA_BIG else orf.EMA_SCHEDULE[-1:]:
        ref = orf.ema_update(s, t, r)["teacher"]
        runs = []
        for with_bf16 in (True, True, False):
            tr, tb = Range(n, lo, fill=t), Range(n, lo, torch.bfloat16)
            ops.ema_update(sd.ptr, tr.ptr, n, r, teacher_bf16=tb.ptr if with_bf16 else None)
            got = held("ema_update", n, f"r={r}", tr, ref, f"lo={lo} bf16={with_bf16}")
            shadow = tb.check("teacher_bf16")
            if with_bf16:
                assert torch.equal(shadow, got.to(torch.bfloat16)), "teacher_bf16 is not bf16 of the teacher the launch wrote"
            else:
                assert bool(torch.isnan(shadow.float()).all()), "teacher_bf16 written though not given"
            runs.append(got)
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), "ema_update differs between launches"
        assert torch.equal(sd.check("student"), s), "ema_update wrote the student"
        if n == N_MUT:
            assert nr.rejected(orf.mutate_ema_exchanged(runs[0], s, t, r), *ref), f"r={r}: r and 1 - r exchanged accepted"
            assert nr.rejected(orf.mutate_ema_neighbour(runs[0], s, t, r), *ref), f"r={r}: the neighbour's teacher accepted"


# ------------------------------------------------------------------------------------------------------------ cast
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 1020, 1023, 1024, 1025, 1028, 1031, 4 * 100003 + 3])
def test_cast_every_length(ops, n):
    src = torch.randn(n, generator=torch.Generator().manual_seed(180)) * 3
    src[0] = 1.0 + 2.0 ** -8                    # a tie: to even
    for lo in (0, 4, 12):
        sr, dst = Range(n, lo, fill=src), Range(n, lo, torch.bfloat16)
        ops.cast_f32_to_bf16(sr.ptr, dst.ptr, n)
        got = dst.check(f"cast n={n} lo={lo}")
        assert torch.equal(got, orf.cast(src)), f"n={n} lo={lo}: not the round-to-nearest-even cast"
        assert torch.equal(sr.check("src"), src)
    note("cast_f32_to_bf16", n, "exact", 0.0)
    if n > 4:
        assert nr.rejected(nr.mutate_truncate_bf16(src), orf.cast(src).double(), torch.zeros(n, dtype=torch.float64))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(ops):
    """n <= 0, n & 3 and NULL operands: WJ_ERR_ARG, and every buffer is left as it was"""
    from wavjepa_amd import _abi
    lib = _abi.load()
    stream = torch.cuda.current_stream().cuda_stream
    n = 1028
    bufs = {k: Range(n, 4) for k in ("p", "g", "m", "v", "out", "ws")}
    b16 = Range(n, 4, torch.bfloat16)
    ptr = {k: b.ptr for k, b in bufs.items()}

    def rc(fn, struct, **fields):
        return getattr(lib, fn)(ctypes.byref(_abi.STRUCTS[struct](**fields)), stream)

    adam = dict(p=ptr["p"], g=ptr["g"], m=ptr["m"], v=ptr["v"], p_bf16=b16.ptr, sumsq=ptr["out"], n=n, lr=4e-4, beta1=0.9, beta2=0.98,
                eps=1e-6, weight_decay=0.04, bc1=0.1, bc2=0.02, max_norm=5.0, grad_scale=1.0, workgroups=0, zero_grad=1)
    for bad in [dict(n=0), dict(n=-4), dict(n=1026), dict(n=1027), dict(p=0), dict(g=0), dict(m=0), dict(v=0)]:
        assert rc("wj_adamw_step", "wj_adamw_args", **{**adam, **bad}) == WJ_ERR_ARG, bad
    ssq = dict(g=ptr["g"], out=ptr["out"], workspace=ptr["ws"], n=n, accumulate=0, workgroups=0)
    for bad in [dict(n=0), dict(n=-4), dict(n=1027), dict(g=0), dict(out=0), dict(workspace=0)]:
        assert rc("wj_grad_sumsq", "wj_sumsq_args", **{**ssq, **bad}) == WJ_ERR_ARG, bad
    ema = dict(student=ptr["g"], teacher=ptr["p"], teacher_bf16=b16.ptr, n=n, r=0.999)
    for bad in [dict(n=0), dict(n=-4), dict(n=1025), dict(student=0), dict(teacher=0)]:
        assert rc("wj_ema_update", "wj_ema_args", **{**ema, **bad}) == WJ_ERR_ARG, bad
    cst = dict(src=ptr["p"], dst=b16.ptr, n=n)
    for bad in [dict(n=0), dict(n=-1), dict(src=0), dict(dst=0)]:
        assert rc("wj_cast_f32_to_bf16", "wj_cast_args", **{**cst, **bad}) == WJ_ERR_ARG, bad
    torch.cuda.synchronize()
    for k, b in list(bufs.items()) + [("p_bf16", b16)]:
        assert bool(torch.isnan(b.check(k).float()).all()), f"a refused call wrote {k}"
