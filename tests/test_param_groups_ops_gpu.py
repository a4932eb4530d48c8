"""wj_adamw_groups_step on the GPU, held per element against tests/param_groups_reference.py (optimizer_reference.adamw_step per group,
its bounds unchanged) and, group by group, bit for bit against wj_adamw_step run with that group's lr / weight decay.

Every launch runs on a sub-range [lo, lo + n) of larger NaN-filled buffers, as FusedAdamW.step calls it on the front-end and side-stream
ranges: lo = granule 0, 1 and 129 of the flat buffer, so that the map offset matters.  n = one granule, two (one byte per wave-lane
pair), 1032 (a second workgroup, one granule into it), 4104 (past four workgroups: `workgroups` = 3 strides) and 262152 (a thousand
workgroups and one granule).  Layouts: one group, two alternating every granule, runs of 1 / 48 / 129 granules, 64 groups, a group that
owns nothing.  workgroups 0 and 3, zero_grad, the bf16 shadow present and NULL, clip active and inactive, grad_scale 0.125, fresh and
warm moments rotate through the cases so that every value meets every layout and every size."""
import ctypes
import itertools

import pytest
import torch

from tests import norm_reference as nr
from tests import optimizer_reference as orf
from tests import param_groups_reference as pgr
from tests.test_optimizer_bounds_gpu import Range, dev, run_sumsq

pytestmark = pytest.mark.gpu

WJ_ERR_ARG = -1
SIZES = (8, 16, 1032, 4104, 262152)
STARTS = (0, 1, 129)                       # first granule of the launch
KINDS = ("randn", "clipped", "scaled", "mixed")
TAIL = 64                                  # elements of the flat buffer behind the range (their map bytes must not be read as the range's)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def cases():
    """(n, start, layout, kind, state, workgroups, zero_grad, with_bf16): every (n, start, layout); the other five rotate with the three
    indices so that each of their values meets every layout, every n and every start (checked below)"""
    out = []
    for (a, n), (b, start), (l, lay) in itertools.product(enumerate(SIZES), enumerate(STARTS), enumerate(pgr.LAYOUTS)):
        out.append((n, start, lay, KINDS[(a + b + l) % 4], orf.STATES[(a + l) % 2], (0, 3)[(a + b) % 2], bool((b + l) % 2), bool((a + b + l) % 3)))
    return out


CASES = cases()


def test_the_cases_cover_every_pairing():
    for col, values in ((3, KINDS), (4, orf.STATES), (5, (0, 3)), (6, (False, True)), (7, (False, True))):
        for fixed in (0, 1, 2):
            for key in {c[fixed] for c in CASES}:
                assert {c[col] for c in CASES if c[fixed] == key} == set(values), (col, fixed, key)


def launch(ops, fn, c, n, lo, sumsq, bufs=None, **kw):
    """one launch of ops.<fn> on fresh guarded copies of the case; returns {p, m, v, g, p_bf16} on the CPU (p_bf16 NaN where not asked for)"""
    r = {k: Range(n, lo, fill=c[k]) for k in ("p", "g", "m", "v")}
    pb = Range(n, lo, torch.bfloat16)
    with_bf16 = kw.pop("with_bf16", True)
    getattr(ops, fn)(r["p"].ptr, r["g"].ptr, r["m"].ptr, r["v"].ptr, n, beta1=pgr.COMMON["beta1"], beta2=pgr.COMMON["beta2"], eps=pgr.COMMON["eps"],
                     step=c["step"], max_norm=pgr.COMMON["max_norm"], sumsq=sumsq, p_bf16=pb.ptr if with_bf16 else None,
                     grad_scale=c["grad_scale"], **kw)
    got = {k: x.check(k) for k, x in r.items()}
    got["p_bf16"] = pb.check("p_bf16")
    return got


@pytest.mark.parametrize("n,start,lay,kind,state,wg,zg,with_bf16", CASES)
def test_grouped_step_on_a_sub_range(ops, n, start, lay, kind, state, wg, zg, with_bf16):
    lo = 8 * start
    gmap, n_groups = pgr.layout(lay, (lo + n + TAIL) // 8)
    emap = gmap.long().repeat_interleave(8)
    elem = emap[lo:lo + n]
    lr, wd = pgr.group_values(n_groups)
    c = orf.adamw_case(kind, state, n, "project", 500 + start)
    Fc = pgr.common_fields(c["step"], c["grad_scale"])
    ss = run_sumsq(ops, c["g"], n, 4 * (lo % 3))
    ssd = ss.to(dev())
    dmap = gmap.to(dev())
    kw = dict(lr=lr, weight_decay=wd, group_map=dmap, first=lo, workgroups=wg, zero_grad=zg, with_bf16=with_bf16)
    got = launch(ops, "adamw_groups_step", c, n, lo, ssd, **kw)
    assert torch.equal(dmap.cpu(), gmap), "the launch wrote its map"
    ref = pgr.grouped_step(c["p"], c["g"], c["m"], c["v"], ss, Fc, lr, wd, elem, zero_grad=zg)
    what = f"n={n} lo={lo} {lay} {kind} / {state} workgroups={wg} zero_grad={zg}"
    for k in ("p", "m", "v", "g") + (("p_bf16",) if with_bf16 else ()):
        ratio = nr.check(got[k], *ref[k], what=f"adamw_groups_step.{k} {what}")
        print(f"adamw_groups_step.{k} {what}: worst error / bound {ratio:.3f}")
    if with_bf16:
        assert torch.equal(got["p_bf16"], got["p"].to(torch.bfloat16)), f"{what}: p_bf16 is not bf16 of the p the launch wrote"
    else:
        assert bool(torch.isnan(got["p_bf16"].float()).all()), f"{what}: the shadow was written without a pointer"
    if zg:
        assert bool((got["g"] == 0).all()), f"{what}: zero_grad left a gradient"
    else:
        assert torch.equal(got["g"], c["g"]), f"{what}: the gradient was written"
    again = launch(ops, "adamw_groups_step", c, n, lo, ssd, **kw)
    for k in got:
        assert torch.equal(got[k].view(torch.int16 if got[k].dtype == torch.bfloat16 else torch.int32),
                           again[k].view(torch.int16 if again[k].dtype == torch.bfloat16 else torch.int32)), f"{what}: {k} differs between two launches"
    # group by group: bit-equal to wj_adamw_step with that group's pair on the same buffers (one group: everywhere)
    present = sorted(set(elem.tolist()))
    assert max(present) < n_groups and (lay != "absent" or 1 not in present)
    for k in present:
        parent = launch(ops, "adamw_step", c, n, lo, ssd, lr=lr[k], weight_decay=wd[k], workgroups=wg, zero_grad=zg, with_bf16=with_bf16)
        sel = elem == k
        for name in ("p", "m", "v", "g") + (("p_bf16",) if with_bf16 else ()):
            a, b = got[name][sel], parent[name][sel]
            bits = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(a.view(bits), b.view(bits)), f"{what}: {name} of group {k} is not bit-equal to wj_adamw_step with its lr / weight decay"
    # the wrong lookups the reference separates are rejected on the kernel's own output
    if n == 1032 and lay != "one":
        muts = pgr.mutations(c["p"], c["g"], c["m"], c["v"], ss, Fc, lr, wd, emap, lo, n, got["p"], ref["p"][1], pair=(0, 2) if lay == "absent" else (0, 1))
        for label, mut, claimed in muts:
            if label == "offset ignored" and (lo == 0 or torch.equal(emap[:n], elem)):
                continue                                         # (nothing to ignore at granule 0, or a layout whose period divides lo)
            assert claimed, f"{what}: mutation '{label}' is not separated by the reference"
            assert nr.rejected(mut, *ref["p"]), f"{what}: mutation '{label}' accepted"


def test_refused_calls_write_nothing(ops):
    from wavjepa_amd import _abi
    lib = _abi.load("optim")
    stream = torch.cuda.current_stream().cuda_stream
    n, lo = 1032, 8
    bufs = {k: Range(n, lo) for k in ("p", "g", "m", "v")}
    b16 = Range(n, lo, torch.bfloat16)
    ss = torch.ones(1, device=dev())
    gmap = torch.zeros((lo + n) // 8, dtype=torch.uint8, device=dev())
    S = _abi.LIBRARIES["optim"].struct_types["wj_adamw_groups_args"]
    table = ctypes.c_float * 64
    good = dict(p=bufs["p"].ptr, g=bufs["g"].ptr, m=bufs["m"].ptr, v=bufs["v"].ptr, p_bf16=b16.ptr, sumsq=ss.data_ptr(), n=n, beta1=0.9,
                beta2=0.98, eps=1e-6, bc1=0.1, bc2=0.02, max_norm=5.0, grad_scale=1.0, workgroups=0, zero_grad=1, n_groups=2,
                lr=table(1e-3, 1e-5), weight_decay=table(0.4, 0.0), group_map=gmap.data_ptr(), first=lo)
    for bad in [dict(n=0), dict(n=-8), dict(n=1028), dict(n=1031), dict(p=0), dict(g=0), dict(m=0), dict(v=0), dict(group_map=0), dict(first=4),
                dict(first=-8), dict(first=12), dict(n_groups=0), dict(n_groups=65), dict(p=bufs["p"].ptr + 4), dict(v=bufs["v"].ptr + 8),
                dict(p_bf16=b16.ptr + 2)]:
        assert lib.wj_adamw_groups_step(ctypes.byref(S(**{**good, **bad})), stream) == WJ_ERR_ARG, bad
    torch.cuda.synchronize()
    for k, b in list(bufs.items()) + [("p_bf16", b16)]:
        assert bool(torch.isnan(b.check(k).float()).all()), f"a refused call wrote {k}"
    assert bool((gmap == 0).all()) and float(ss) == 1.0
