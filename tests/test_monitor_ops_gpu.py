"""wj_masked_moments on the GPU: every kernel case of tests/moments_reference.py in the dense, ragged and trimmed row forms, held to the
check that rejects the mutations (tests/test_monitor_cpu.py): per-column variance and both scalars inside the bound, the constant
column's M2 exactly 0, n exact.  Operands start one row (preds, targets), one byte (tgt) or one element (rows) behind their
allocation; out, col and the workspace lie between NaN guards; two launches give the same bits."""
import pytest
import torch

from tests import moments_reference as mr
from tests import norm_reference as nr
from tests.test_jepa_gpu import dev

pytestmark = pytest.mark.gpu

N_CASES = len(mr.SHAPES) + 3


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


@pytest.fixture(scope="module")
def cases(ops):
    """[(name, case, {form: bounds})], computed once"""
    return [(name, case, {form: mr.bounds(case, form) for form in mr.FORMS}) for name, case in mr.kernel_cases(ops.MOMENTS_ROWS)]


def behind(t: torch.Tensor, lead: int) -> torch.Tensor:
    """t on the device, `lead` elements (rows of a matrix) behind the start of its allocation"""
    buf = torch.zeros((t.shape[0] + lead + 1,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev())
    buf[lead:lead + t.shape[0]] = t.to(dev())
    return buf[lead:lead + t.shape[0]]


def launch(ops, case, form, with_col=True):
    B, G, T, D = (case[k] for k in "BGTD")
    rows = None if form == "dense" else mr.row_list(case, form)
    preds, targets = behind(mr.packed_preds(case, form), 1), behind(case["targets"], 1)
    tgt = behind(case["tgt"], 1)
    assert tgt.data_ptr() % 2 == 1 and preds.data_ptr() % 16 == 0 and targets.data_ptr() % 16 == 0
    kw = {}
    if rows is not None:
        kw = dict(rows=behind(rows, 1), n_rows=len(rows))
        assert kw["rows"].data_ptr() % 8 == 4
    need = ops.workspace_bytes("wj_masked_moments", B=B, G=G, T=T, D=D, n_rows=0 if rows is None else len(rows))
    out, col, ws = nr.Guarded(4, None, torch.float32, dev()), nr.Guarded(4 * D, None, torch.float64, dev()), nr.Guarded(need // 8, None, torch.float64, dev())
    ops.masked_moments(preds, targets, tgt, out.view, ws.view, B=B, G=G, T=T, D=D, col=col.view if with_col else None, **kw)
    torch.cuda.synchronize()
    what = f"masked_moments {B, G, T, D} {form}"
    ws.check("workspace " + what)
    o = out.check("out " + what).cpu()
    c = col.check("col " + what).cpu()
    if not with_col:
        assert bool(torch.isnan(c).all()), f"{what}: col written though not asked for"
    assert not bool(torch.isnan(o).any()) and float(o[3]) == 0.0, what
    return o, c.view(2, 2, D)


@pytest.mark.parametrize("form", mr.FORMS)
@pytest.mark.parametrize("idx", range(N_CASES))
def test_masked_moments_kernel(ops, cases, idx, form):
    name, case, bnds = cases[idx]
    bnd = bnds[form]
    o, c = launch(ops, case, form)
    o2, c2 = launch(ops, case, form)
    assert torch.equal(o, o2) and torch.equal(c, c2), f"{name} {form}: two launches differ"
    o3, _ = launch(ops, case, form, with_col=False)
    assert torch.equal(o, o3), f"{name} {form}: the scalars depend on col"
    got = dict(n=float(o[2]), mean=[c[0, 0].numpy(), c[1, 0].numpy()], M2=[c[0, 1].numpy(), c[1, 1].numpy()],
               pred_var=float(o[0]), target_var=float(o[1]))
    ref = bnd["ref"]
    print(f"{name} {form}: n {got['n']:.0f}  pred_var {got['pred_var']!r} (reference {ref['pred_var']!r})  target_var {got['target_var']!r} "
          f"(reference {ref['target_var']!r})  bounds {bnd['bound_stat'][0]:.3e} {bnd['bound_stat'][1]:.3e}")
    assert mr.violations(got, case, form, bnd) == [], (name, form)
    for q in (0, 1):                                            # the means a data-parallel merge starts from
        assert abs(got["mean"][q] - ref["mean"][q]).max() <= 1e-12 * max(1.0, abs(ref["mean"][q]).max()), (name, form, q)
    if case["D"] > mr.COL_SPIKE and got["n"] >= 2:
        assert got["M2"][0][mr.COL_SPIKE] > 1e5 and got["M2"][1][mr.COL_SPIKE] > 1e5      # the row holding 1e3 is among the targets


def test_single_target_row_has_variance_zero(ops, cases):
    name, case, _ = cases[0]
    assert (case["B"], case["G"], case["T"], case["D"]) == (1, 1, 1, 8)
    for form in mr.FORMS:
        o, c = launch(ops, case, form)
        assert float(o[2]) == 1.0 and float(o[0]) == float(o[1]) == float(torch.tensor(1e-6, dtype=torch.float64).sqrt().float())
        assert bool((c[:, 1] == 0).all())
        assert torch.equal(c[0, 0], case["preds"][0].double()) and torch.equal(c[1, 0], case["targets"][0].double())
