"""The optimiser-pass reference helper (tests/optimizer_reference.py) on the host.

  * its fp64 single-step AdamW, chained over 20 steps, reproduces torch.optim.AdamW in float64 behind clip_grad_norm_ (with and without
    clipping, with and without weight decay) to 1e-12 per element: the semantics are anchored to torch, not to the project's kernel;
  * an fp32 numpy emulation in the kernels' order stays below MARGIN of every bound, for every kind x state x size (printed);
  * every claimed mutation is rejected on the emulation's output, and every REQUIRED (mutation, kind, state) triple is claimed;
  * the reference program's EMA wording stays inside the bound of the header's over the schedule of r;
  * every field of the four argument structs is handled by the reference or named in its exclusion list.
"""
import collections

import numpy as np
import pytest
import torch

from tests import norm_reference as nr
from tests import optimizer_reference as orf
from wavjepa_amd import _abi

MARGIN = 0.8
SIZES = (4, 1020, 1028, 4 * 100003)
SUMSQ_BIG = 4 * (1024 * 256 + 77)
EMA_BIG = 4 * (8192 * 256 + 77)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------------------------------------------------ torch float64
@pytest.mark.parametrize("max_norm,wd,scale", [(5.0, 0.04, 1e-2), (5.0, 0.04, 3.0), (0.0, 0.04, 3.0), (5.0, 0.0, 3.0)])
def test_chained_reference_reproduces_torch_adamw_in_float64(max_norm, wd, scale):
    n, steps = 257, 20
    H = dict(lr=4e-4, beta1=0.9, beta2=0.98, eps=1e-6, weight_decay=wd, max_norm=max_norm)
    gen = torch.Generator().manual_seed(5)
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    pref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pref], lr=H["lr"], betas=(H["beta1"], H["beta2"]), eps=H["eps"], weight_decay=wd, foreach=False)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    clipped = 0
    for step in range(1, steps + 1):
        g = scale * torch.randn(n, generator=gen, dtype=torch.float64)
        pref.grad = g.clone()
        if max_norm > 0:
            clipped += float(torch.nn.utils.clip_grad_norm_([pref], max_norm)) > max_norm
        opt.step()
        # the fields in double: this test holds the formula, not the rounding of the fields
        Fd = dict(lr=H["lr"], beta1=H["beta1"], beta2=H["beta2"], eps=H["eps"], weight_decay=wd, bc1=1 - H["beta1"] ** step,
                  bc2=1 - H["beta2"] ** step, max_norm=max_norm, grad_scale=1.0)
        r = orf._adamw(p, g, m, v, (g * g).sum().reshape(1), Fd)
        p, m, v = r["p"], r["m"], r["v"]
        st = opt.state[pref]
        assert float(((p - pref.detach()).abs() / pref.detach().abs()).max()) < 1e-12, step
        assert float(((m - st["exp_avg"]).abs() / (r["t1"].abs() + r["t2"].abs())).max()) < 1e-12, step
        assert float(((v - st["exp_avg_sq"]).abs() / v).max()) < 1e-12, step
    assert clipped == (steps if (max_norm > 0 and scale > 1) else 0)


# ------------------------------------------------------------------------------------------------------------ margin
def emulated(c, Fd, n):
    ss = t(orf.emulate_sumsq(c["g"]))
    return ss, orf.emulate_adamw(c["p"], c["g"], c["m"], c["v"], ss, Fd)


def test_emulation_stays_below_the_margin_of_every_bound():
    w = collections.defaultdict(float)
    for n in SIZES:
        for hyper in orf.HYPER:
            for i, kind in enumerate(orf.KINDS):
                for state in orf.STATES:
                    c = orf.adamw_case(kind, state, n, hyper, 10 + i)
                    Fd = orf.fields(c["H"], c["step"], c["grad_scale"])
                    ss, got = emulated(c, Fd, n)
                    w["sumsq"] = max(w["sumsq"], nr.worst(ss, *orf.grad_sumsq(c["g"])["out"]))
                    ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd)
                    for k in ("p", "m", "v", "p_bf16", "g"):
                        w[k] = max(w[k], nr.worst(t(got[k]), *ref[k]))
                    # the kinds are what they say
                    _, active = orf._clip(ss, Fd)
                    if kind != "mixed":         # (its norm is whatever twelve decades of magnitude give)
                        assert active == (kind in ("clipped", "scaled")), (kind, n)
                    if kind == "scaled":
                        assert orf._clip(ss, Fd, "clip_unscaled")[0] < 0.5 * orf._clip(ss, Fd)[0]
                    if kind == "tiny" and n > 4:
                        assert float(ref["v"][0].sqrt().median()) <= Fd["eps"]
    for n in SIZES + (SUMSQ_BIG,):
        g, _ = orf.make_grad("randn", n, 31, orf.HYPER["project"])
        for wg in (0, 1, 3):
            out0 = torch.tensor([0.37])
            for acc in (False, True):
                got = orf.emulate_sumsq(g, out0, acc, wg)
                w["sumsq"] = max(w["sumsq"], nr.worst(t(got), *orf.grad_sumsq(g, out0, acc)["out"]))
    for n in SIZES:
        s, te = orf.ema_case(n, 41)
        for r in orf.EMA_SCHEDULE:
            ref = orf.ema_update(s, te, r)["teacher"]
            w["ema"] = max(w["ema"], nr.worst(t(orf.emulate_ema(s, te, r)), *ref))
    print()
    for k, v in w.items():
        print(f"emulation / bound  {k:10s} {v:.3f}")
    over = {k: v for k, v in w.items() if not v < MARGIN}
    assert not over, f"emulation above {MARGIN} of the bound: {over}"


def test_reference_program_ema_wording_stays_inside_the_bound():
    """teacher.mul_(r).add_((1 - r) student) with 1 - r formed in double: its coefficient differs from 1 - float32(r) by up to 0.14 %,
    a fraction of u |s| per element.  In fp64 (the difference of the formulas alone) and in fp32 (with its own roundings)."""
    s, te = orf.ema_case(4 * 100003, 43)
    print()
    for r in orf.EMA_SCHEDULE:
        r32 = nr.f32eps(r)
        in_u = abs(nr.f32eps(1.0 - r) - (1.0 - r32)) / nr.U
        ref = orf.ema_update(s, te, r)["teacher"]
        w64 = nr.worst(orf.ema_update_program(s, te, r), *ref)
        w32 = nr.worst(t(orf.emulate_ema_program(s, te, r)), *ref)
        print(f"r = {r}: coefficient off by {in_u:.2f} u; program form / bound {w64:.3f} (fp64) {w32:.3f} (fp32)")
        assert in_u < 0.5 and w64 < 0.5 and w32 < 1.0


# ------------------------------------------------------------------------------------------------------------ mutations
def test_mutations_are_rejected_on_the_emulation():
    n, count = 1028, 0
    claimed_somewhere = set()
    for hyper in orf.HYPER:
        for i, kind in enumerate(orf.KINDS):
            for state in orf.STATES:
                c = orf.adamw_case(kind, state, n, hyper, 20 + i)
                Fd = orf.fields(c["H"], c["step"], c["grad_scale"])
                ss, got = emulated(c, Fd, n)
                ref = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, Fd)
                got = {k: t(v) for k, v in got.items()}
                for k in ("p", "m", "v", "p_bf16"):
                    nr.check(got[k], *ref[k], what=f"{kind} {state} {k}")
                muts = orf.adamw_mutations(c, ss, Fd, got, ref)
                assert not orf.required_missing(c, muts), orf.required_missing(c, muts)
                for label, k, m, cl in muts:
                    if cl:
                        assert nr.rejected(m, *ref[k]), f"{hyper} {kind} {state}: {label} ({k}) accepted"
                        claimed_somewhere.add(label)
                        count += 1
    assert claimed_somewhere == set(orf.FORMULAS) | {"stale vector", "vectors swapped", "bf16 truncated"}
    assert count > 300
    # sumsq
    for n in (4, 1020, 1028, 4 * 100003, 2 ** 20):
        g, _ = orf.make_grad("randn", n, 31, orf.HYPER["project"])
        assert orf.sumsq_last_vector_separates(g), n           # 4 g^2 > KAPPA u sum g^2 up to n = 2^20
        got, ref = t(orf.emulate_sumsq(g)), orf.grad_sumsq(g)["out"]
        nr.check(got, *ref, what="sumsq")
        assert nr.rejected(orf.mutate_sumsq_drop_last(got, g), *ref), f"n={n}: last vector dropped accepted"
        out0 = torch.tensor([0.5 * float(ref[0])])
        got, ref = t(orf.emulate_sumsq(g, out0, True)), orf.grad_sumsq(g, out0, True)["out"]
        nr.check(got, *ref, what="sumsq accumulate")
        assert nr.rejected(orf.mutate_sumsq_ignore_out0(got, out0), *ref), f"n={n}: out0 ignored accepted"
    # EMA
    s, te = orf.ema_case(1028, 45)
    for r in orf.EMA_SCHEDULE:
        got, ref = t(orf.emulate_ema(s, te, r)), orf.ema_update(s, te, r)["teacher"]
        nr.check(got, *ref, what="ema")
        assert nr.rejected(orf.mutate_ema_exchanged(got, s, te, r), *ref), f"r={r}: r and 1 - r exchanged accepted"
        assert nr.rejected(orf.mutate_ema_neighbour(got, s, te, r), *ref), f"r={r}: the neighbour's teacher accepted"


def test_cast_reference_is_round_to_nearest_even():
    x = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0e38, 1e-40])
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0e38, 1e-40]).to(torch.bfloat16)
    assert torch.equal(orf.cast(x), want)


# ------------------------------------------------------------------------------------------------------------ coverage gate
def test_every_field_of_the_argument_structs_is_handled_or_excluded():
    assert set(orf.HANDLED) == {"wj_adamw_args", "wj_sumsq_args", "wj_ema_args", "wj_cast_args"}
    for name, handled in orf.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        excluded = set(orf.EXCLUDED.get(name, {}))
        assert not (handled & excluded), name
        assert fields - handled - excluded == set(), f"{name}: fields without a reference or an exclusion: {sorted(fields - handled - excluded)}"
        assert (handled | excluded) - fields == set(), f"{name}: listed but not in the header: {sorted((handled | excluded) - fields)}"
