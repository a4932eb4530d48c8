"""wj_gemm_bf16_act on the GPU, single launches: every bf16 input through both epilogue forms of each schedule, random operands against
the fp64 reference of tests/act_reference.py (outputs NaN-filled between guard bands), launch-to-launch identity, WJ_ACT_GELU against
wj_gemm_bf16 bit for bit, and the mutations applied to what the GPU wrote."""
import pytest
import torch

from tests import act_reference as R
from tests import gemm_reference as gr

pytestmark = pytest.mark.gpu
SCHEDULES = (0, 3, 4)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda")


def _ordinal(t):                                                              # bf16 bits -> integers ordered like the values
    b = t.view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(b >= 0x8000, 0x8000 - b, b)


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_every_bf16_input_through_both_forms(ops, kind, schedule):
    """h = bf16(0 + bias) with A = 0: every finite bf16 value (+-0, subnormals, the largest magnitudes) is one column's h; 256 rows x
    65 536 columns are 256 work items, what the persistent schedule needs to be taken.  Everything finite; ReLU equal to the reference;
    the other two inside the bound; where act' has saturated it is exactly 1 / 0."""
    vals = R.every_bf16()
    ok = torch.isfinite(vals)
    N, M, K = 65536, 256, 128
    bias = torch.where(ok, vals, torch.zeros_like(vals)).to(dev())
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=dev())
    W = (torch.randn(N, K, generator=torch.Generator().manual_seed(70)) * 0.05).to(torch.bfloat16).to(dev())
    kw = dict(act=kind, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, schedule=schedule)
    d1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    g2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    g1 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
    ops.gemm_act(A, W, d1, C2=g2, epilogue=ops.EPI_BIAS_GELU2, **kw)
    ops.gemm_act(A, W, g1, epilogue=ops.EPI_BIAS_GELU, **kw)
    torch.cuda.synchronize()
    assert torch.equal(g1.view(torch.int16), g2.view(torch.int16))            # both forms store the same act(h)
    for t in (d1, g2):
        assert bool((t.view(torch.int16) == t[0].view(torch.int16)).all())    # every row the same bits
    act, act1 = g2[0].cpu()[ok], d1[0].cpu()[ok]
    v = vals[ok]
    assert bool(torch.isfinite(act.float()).all() and torch.isfinite(act1.float()).all())
    normal = (v.abs() >= 2.0 ** -126) | (v == 0)
    if kind == "relu":
        f, f1, _ = R.act_fns(kind, v)
        assert torch.equal(act.double()[normal], f[normal]) and torch.equal(act1.double()[normal], f1[normal])
        assert bool((act1[v == 0] == 0).all())
    fails, worst = R.check(kind, v.double(), act, act1)
    assert not fails, (schedule, fails)
    assert bool((act1[v >= 64.0].float() == 1.0).all()) and bool((act1[v <= -128.0].float() == 0.0).all())
    assert torch.equal(act[v >= 64.0].view(torch.int16), v[v >= 64.0].to(torch.bfloat16).view(torch.int16))
    if kind != "relu":
        f, f1, _ = R.act_fns(kind, v)
        off = [int((_ordinal(g) != _ordinal(r.float().to(torch.bfloat16)))[normal].sum()) for g, r in ((act, f), (act1, f1))]
        print(f"{kind} schedule {schedule}: not the correctly rounded fp64 value on {off[0]} (act) / {off[1]} (act') of {int(normal.sum())} "
              f"inputs; worst |got - ref| / bound {worst:.3f}")


def _fields(M, N, K, ldc, two):
    return dict(entry="gemm", unknown=(), M=M, N=N, K=K, lda=K, ldb=K, ldc=ldc, epilogue="BIAS_GELU2" if two else "BIAS_GELU", bias=True,
                C=True, C2=two, align=(), a_trans=0, b_trans=0, split_k=1, seg_rows=0, seg_valid=0, alpha=1.0, aux=False, colsum=False,
                rowmap=None, workspace=False, schedule=None, persist_cus=None)


SHAPES = [(256, 256, 128, 256, 0), (256, 256, 128, 256, 3), (300, 384, 128, 384, 0), (300, 384, 128, 384, 3), (300, 384, 128, 512, 0),
          (20000, 1024, 384, 1024, 4), (16500, 1152, 128, 1152, 4), (9000, 2432, 128, 2432, 4)]      # 2432 % 256 == 128: the half-width item


@pytest.mark.parametrize("M, N, K, ldc, schedule", SHAPES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_random_operands_against_fp64(ops, kind, M, N, K, ldc, schedule):
    for two in (True, False):
        f = _fields(M, N, K, ldc, two)
        o = gr.Operands(f, dev(), seed=5, a_scale=1.0, b_scale=0.08)
        o.b["A"].rows(0, 1, K, K).zero_()                                 # a planted h == 0: a zero row of A under a zero bias
        o.b["bias"].t[o.b["bias"].p] = 0.0
        kw = {k: v for k, v in o.kwargs().items() if k in ("A", "B", "C", "C2", "bias", "M", "N", "K", "lda", "ldb", "ldc", "epilogue")}
        o.reset_outputs()
        snap = o.snapshot()
        ops.gemm_act(act=kind, schedule=schedule, **kw)
        torch.cuda.synchronize()
        first = {n: o.b[n].t.clone() for n in snap}
        o.reset_outputs()
        ops.gemm_act(act=kind, schedule=schedule, **kw)
        torch.cuda.synchronize()
        for n in snap:                                                    # two launches: the same bits, guard bands included
            assert torch.equal(gr._ibits(first[n]), gr._ibits(o.b[n].t)), n
        acc, sab = gr.accumulate(o, 0, M)
        bias = o.epi_inputs(0, M)["bias"]
        v, err = acc + bias, gr.KAPPA * gr.U * sab + gr.U * bias.abs()
        act = o.region("C2" if two else "C")
        act1 = o.region("C") if two else None
        fails, worst = R.check(kind, v, act, None if kind == "relu" else act1, err)
        assert not fails, (two, fails)
        zero = (v == 0) & (err == 0)
        assert bool(zero[0, 0])
        if kind == "relu" and two:
            assert torch.equal(act1.float(), (act.float() > 0).float())
            assert bool((act1[zero] == 0).all()) and bool((act[zero] == 0).all())         # 0 at h == 0, as torch
        for n, s in snap.items():                                         # nothing outside the output region changed
            t = o.b[n].t.clone()
            o.set_region(n, o.region(n, s), t)
            assert torch.equal(gr._ibits(t), gr._ibits(s)), f"{n}: bytes outside the output region changed"
        if (M, N, ldc) == (300, 384, 384) and two:
            names = []
            for name, ma, m1 in R.mutations(kind, gr.bf16(v), act.clone(), act1.clone()):
                names.append(name)
                if kind == "relu" and "swapped" not in name:              # the planted zero: the exact rule above rejects it
                    bad = bool((m1[zero] != 0).any())
                else:
                    bad = R.check(kind, v, ma, None if kind == "relu" else m1, err)[0]
                assert bad, f"{kind}: mutation of the GPU's outputs not rejected: {name}"
            assert len(names) >= 2


@pytest.mark.parametrize("M, N, K, schedule", [(300, 384, 128, 0), (300, 384, 128, 3), (512, 256, 256, 3), (20000, 1024, 384, 4), (9000, 2432, 128, 4)])
def test_gelu_through_the_new_entry_is_wj_gemm_bf16(ops, M, N, K, schedule):
    g = torch.Generator().manual_seed(9)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(dev())
    W = (torch.randn(N, K, generator=g) * 0.08).to(torch.bfloat16).to(dev())
    bias = torch.randn(N, generator=g).to(dev())
    for epi, two in ((ops.EPI_BIAS_GELU2, True), (ops.EPI_BIAS_GELU, False)):
        out = []
        for fn, extra in ((ops.gemm, {}), (ops.gemm_act, dict(act="gelu"))):
            C = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev())
            C2 = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev()) if two else None
            fn(A, W, C, C2=C2, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias, epilogue=epi, schedule=schedule, **extra)
            torch.cuda.synchronize()
            out.append((C, C2))
        assert torch.equal(out[0][0].view(torch.int16), out[1][0].view(torch.int16))
        assert not two or torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16))
        assert not bool(torch.isnan(out[1][0].float()).any())
