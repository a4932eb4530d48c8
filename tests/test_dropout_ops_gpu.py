"""The five dropout entries, one launch at a time, against the host's bit-exact masks (tests/dropout_reference.py).

wj_dropout_rows is held bit for bit (one fp32 multiply and one rounding are reproducible on the host); the LayerNorm pair against fp64
torch math with the helper's mask at the bounds of tests/test_ops_gpu.py::test_layernorm_fwd_bwd; the attention pair against
tests/attention_reference.py's fp64 result and per-element bound with P o m in place of P (KAPPA unchanged).  Every output sits between
NaN-filled guard bands, two launches are bit-identical, and the mutations a subtly wrong kernel would make are rejected by the same
checks at T = 129 and (67, 384)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import attention_reference as ar
from tests import dropout_reference as R

pytestmark = pytest.mark.gpu

SEED, CALL = 0x1234_5678_9ABC_DEF1, 7
GUARD = 256


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


def rnd(*shape, dtype=torch.float32, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def relerr(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Guarded:
    """a tensor inside a larger NaN-filled allocation"""

    def __init__(self, shape, dtype, init=None):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev())
        self.t = self.full[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def guards_intact(self):
        return bool(torch.isnan(self.full[:GUARD]).all()) and bool(torch.isnan(self.full[-GUARD:]).all())


def binomial_ok(keep: torch.Tensor, p: float) -> bool:
    pe = R.thr_scale(p)[0] / 65536.0
    n = keep.numel()
    return abs(float(keep.double().mean()) - (1 - pe)) <= 5 * math.sqrt(pe * (1 - pe) / n)


# ---------------------------------------------------------------------------------------------------------------- wj_dropout_rows
@pytest.mark.parametrize("p", [0.1, 0.5, 1 / 65536])
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("M,N", [(1, 8), (67, 1536), (400, 3072), (1031, 256)])
def test_dropout_rows_bit_for_bit(ops, M, N, two, p):
    x0, y0 = rnd(M, N, dtype=torch.bfloat16, seed=1), rnd(M, N, dtype=torch.bfloat16, seed=2)
    keep = torch.from_numpy(R.row_keep(SEED, CALL, 1, 3, R.SITE_FFN, M, N, p)).to(dev())
    scale = torch.tensor(float(R.thr_scale(p)[1]), dtype=torch.float32, device=dev())
    drop = ops.drop_args(SEED, CALL, p, site=R.SITE_FFN, layer=3, stack=1)
    runs = []
    for _ in range(2):
        x, y = Guarded((M, N), torch.bfloat16, x0), Guarded((M, N), torch.bfloat16, y0)
        ops.dropout_rows(x.t, y.t if two else None, M=M, N=N, drop=drop)
        torch.cuda.synchronize()
        assert x.guards_intact() and y.guards_intact()
        runs.append((x.t.clone(), y.t.clone()))
    assert torch.equal(runs[0][0].view(torch.int16), runs[1][0].view(torch.int16))
    for got, src in ((runs[0][0], x0), (runs[0][1], y0)) if two else ((runs[0][0], x0),):
        want = torch.where(keep, (src.float() * scale).to(torch.bfloat16), torch.zeros_like(src))     # +0 where dropped
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    if not two:
        assert torch.equal(runs[0][1].view(torch.int16), y0.view(torch.int16))
    if M * N >= 100000:
        assert binomial_ok(runs[0][0] != 0, p) or p < 1e-3
        assert binomial_ok(keep, p)


# ---------------------------------------------------------------------------------------------------------------- LayerNorm pair
def _ln_case(ops, M, D, p=0.1, keep=None, scale=None, site=R.SITE_RES1, layer=2, stack=0):
    """one forward + backward launch pair; returns everything the checks need"""
    x, r = rnd(M, D, seed=20), rnd(M, D, dtype=torch.bfloat16, seed=21)
    gamma, beta, dy = 1 + 0.1 * rnd(D, seed=22), 0.1 * rnd(D, seed=23), rnd(M, D, seed=24)
    drop = ops.drop_args(SEED, CALL, p, site=site, layer=layer, stack=stack)
    out = {}
    for run in range(2):
        y, yb = Guarded((M, D), torch.float32), Guarded((M, D), torch.bfloat16)
        mean, rstd = Guarded((M,), torch.float32), Guarded((M,), torch.float32)
        ops.layernorm_fwd_drop(x, gamma, beta, M=M, D=D, eps=1e-6, r=r, y_f32=y.t, y_bf16=yb.t, mean=mean.t, rstd=rstd.t, drop=drop)
        ds, dsb = Guarded((M, D), torch.float32), Guarded((M, D), torch.bfloat16)
        dg, db, dbi = (Guarded((D,), torch.float32, torch.zeros(D)) for _ in range(3))
        wsp = torch.empty(1536 * 3 * D, device=dev())
        ops.layernorm_bwd_drop(dy, x, gamma, mean.t, rstd.t, M=M, D=D, r=r, ds_f32=ds.t, ds_bf16=dsb.t, dgamma=dg.t, dbeta=db.t, dbias=dbi.t,
                               workspace=wsp, drop=drop)
        torch.cuda.synchronize()
        for g in (y, yb, mean, rstd, ds, dsb, dg, db, dbi):
            assert g.guards_intact()
        out[run] = dict(y=y.t, yb=yb.t, ds=ds.t, dsb=dsb.t, dg=dg.t, db=db.t, dbi=dbi.t)
    for k in ("y", "yb", "ds", "dsb"):                          # (the column sums meet in float atomics: not bit-reproducible by design)
        assert torch.equal(out[0][k].view(torch.int32 if out[0][k].dtype == torch.float32 else torch.int16),
                           out[1][k].view(torch.int32 if out[1][k].dtype == torch.float32 else torch.int16)), k
    return dict(out[0], x=x, r=r, gamma=gamma, beta=beta, dy=dy)


def _ln_reference(c, keep, scale, D):
    """fp64 torch math: s = x + r o m * scale, y = LN(s); gradients of (y * dy).sum()"""
    xr = c["x"].double().requires_grad_(True)
    rr = c["r"].double().requires_grad_(True)
    g2, b2 = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    ref = F.layer_norm(xr + rr * keep.double() * float(scale), (D,), g2, b2, 1e-6)
    ref.backward(c["dy"].double())
    return ref, xr.grad, rr.grad, g2.grad, b2.grad


def _ln_failures(c, ref, keep, scale, M, D):
    """the assertions of test_layernorm_fwd_bwd, at its bounds, as a list of what fails"""
    y_ref, dx, dr, dgam, dbet = ref
    sc = torch.tensor(float(scale), dtype=torch.float32, device=dev())
    bad = []
    if not relerr(c["y"], y_ref) < 1e-5:
        bad.append(f"y {relerr(c['y'], y_ref):.3g}")
    if not torch.equal(c["yb"], c["y"].to(torch.bfloat16)):
        bad.append("y_bf16 is not the rounded y_f32")
    if not relerr(c["ds"], dx) < 2e-5:
        bad.append(f"ds_f32 {relerr(c['ds'], dx):.3g}")
    if not relerr(c["dg"], dgam) < 2e-5 or not relerr(c["db"], dbet) < 2e-5:
        bad.append(f"dgamma / dbeta {relerr(c['dg'], dgam):.3g} {relerr(c['db'], dbet):.3g}")
    if float(c["dsb"][~keep].float().abs().max() if bool((~keep).any()) else 0.0) != 0.0:
        bad.append("ds_bf16 not exactly 0 at dropped positions")
    want = torch.where(keep, (c["ds"] * sc).to(torch.bfloat16), torch.zeros_like(c["dsb"]))
    if not torch.equal(c["dsb"], want):
        bad.append("ds_bf16 is not bf16(ds o m * scale)")
    if not relerr(c["dsb"].float(), dr) < 4e-3:                  # bf16 resolution on top of the fp64 gradient of r
        bad.append(f"ds_bf16 against d r {relerr(c['dsb'].float(), dr):.3g}")
    if not relerr(c["dbi"], c["dsb"].float().sum(0)) < 1e-5:
        bad.append(f"dbias {relerr(c['dbi'], c['dsb'].float().sum(0)):.3g}")
    return bad


@pytest.mark.parametrize("M,D", [(1, 64), (11, 128), (67, 384), (37, 768), (9, 1024), (400, 768)])
def test_layernorm_pair_against_fp64(ops, M, D):
    p = 0.1
    keep = torch.from_numpy(R.row_keep(SEED, CALL, 0, 2, R.SITE_RES1, M, D, p)).to(dev())
    scale = R.thr_scale(p)[1]
    c = _ln_case(ops, M, D, p)
    bad = _ln_failures(c, _ln_reference(c, keep, scale, D), keep, scale, M, D)
    assert not bad, bad
    if M * D >= 100000:
        assert binomial_ok(c["dsb"] != 0, p)


def test_layernorm_pair_rejects_the_mutations(ops):
    """(67, 384): the launch's outputs against references built with a wrong mask or scale -- each must fail the checks above."""
    M, D, p = 67, 384, 0.1
    scale = float(R.thr_scale(p)[1])
    keep = torch.from_numpy(R.row_keep(SEED, CALL, 0, 2, R.SITE_RES1, M, D, p)).to(dev())
    c = _ln_case(ops, M, D, p)
    assert not _ln_failures(c, _ln_reference(c, keep, scale, D), keep, scale, M, D)
    wrong = {"no scale": (keep, 1.0), "scale twice": (keep, scale * scale),
             "no mask": (torch.ones_like(keep), scale),
             "another layer's mask": (torch.from_numpy(R.row_keep(SEED, CALL, 0, 3, R.SITE_RES1, M, D, p)).to(dev()), scale),
             "another site's mask": (torch.from_numpy(R.row_keep(SEED, CALL, 0, 2, R.SITE_RES2, M, D, p)).to(dev()), scale),
             "another call's mask": (torch.from_numpy(R.row_keep(SEED, CALL + 1, 0, 2, R.SITE_RES1, M, D, p)).to(dev()), scale)}
    for what, (k, s) in wrong.items():
        assert _ln_failures(c, _ln_reference(c, k, s, D), k, s, M, D), f"mutation '{what}' was not rejected"
    # the mask missing from ds_bf16 only: a kernel that stored bf16(ds) as the parent does
    c2 = dict(c, dsb=c["ds"].to(torch.bfloat16))
    assert _ln_failures(c2, _ln_reference(c, keep, scale, D), keep, scale, M, D)


# ---------------------------------------------------------------------------------------------------------------- attention pair
def _forms(B, T):
    g = np.random.default_rng(T)
    out = [ar.fields(B, T, 2, 0, "none")]
    if T > 1:
        m = g.random((B, T)) < 0.3
        m[:, 0] = False
        out.append(ar.fields(B, T, 2, 0, "mask", mask=m))
        out.append(ar.fields(B, T, 2, 0, "mask", mask=m[:1], mask_group=3))
    return out


def _keep_scale(B, H, T, p, layer=1, stack=0, transpose=False, one_head=False, call=CALL):
    k = R.attn_keep(SEED, call, stack, layer, B, H, T, T, p)
    if transpose:
        k = np.ascontiguousarray(k.transpose(0, 1, 3, 2))
    if one_head:
        k = np.repeat(k[:, :1], H, axis=1)
    return torch.from_numpy(k).to(dev())


def _attn_launch(ops, o, p, det=False, layer=1):
    drop = ops.drop_args(SEED, CALL, p, site=R.SITE_ATTN, layer=layer, stack=0)
    snap_f = o.snapshot("fwd")
    ops.attn_stream_fwd_drop(**o.fwd_kwargs(), drop=drop)
    torch.cuda.synchronize()
    outs_f = {n: o.b[n].t.clone() for n in snap_f}
    snap_b = o.snapshot("bwd")
    ops.attn_stream_bwd_drop(**o.bwd_kwargs(False), drop=drop, deterministic=det)
    torch.cuda.synchronize()
    outs_b = {n: o.b[n].t.clone() for n in snap_b}
    return snap_f, outs_f, snap_b, outs_b


def _attn_case(ops, f, p=0.1, regime="flat"):
    fails = []
    B, T, H = f["B"], f["T"], f["H"]
    o = ar.Operands(f, dev(), seed=3, regime=regime)
    ks = _keep_scale(B, H, max(o.ix.Tm, 1), p).double() * float(R.thr_scale(p)[1])
    snap_f, outs_f, snap_b, outs_b = _attn_launch(ops, o, p)
    ex_f = R.reference_fwd_drop(ar, o, ks)
    fails += [f"forward: {b}" for b in ar.check(o, ex_f, snap_f, "fwd")[0]]
    ex_b = R.reference_bwd_drop(ar, o, ex_f, ks)
    fails += [f"backward: {b}" for b in ar.check(o, ex_b, snap_b, "bwd", folded=True)[0]]
    # a second launch pair, and two more deterministic backwards: bit-identical
    o.reset_outputs()
    _, again_f, _, again_b = _attn_launch(ops, o, p)
    for n in outs_f:
        if not torch.equal(ar._ibits(outs_f[n]), ar._ibits(again_f[n])):
            fails.append(f"two forward launches differ in {n}")
    if not torch.equal(ar._ibits(outs_b["dqkv"]), ar._ibits(again_b["dqkv"])):
        fails.append("two backward launches differ in dqkv")
    det = []
    for _ in range(3):
        o.reset_outputs("bwd")
        det.append(_attn_launch_bwd_only(ops, o, p))
    for d in det[1:]:
        for n in det[0]:
            if not torch.equal(ar._ibits(det[0][n]), ar._ibits(d[n])):
                fails.append(f"deterministic backward launches differ in {n}")
    # lse is the parent's, bit for bit
    lse_drop = o.b["lse"].t.clone()
    o.reset_outputs("fwd")
    ops.attn_stream_fwd(**o.fwd_kwargs())
    torch.cuda.synchronize()
    if not torch.equal(ar._ibits(lse_drop), ar._ibits(o.b["lse"].t)):
        fails.append("lse differs from the launch without dropout")
    return o, ex_f, ex_b, (snap_f, outs_f, snap_b, outs_b), fails


def _attn_launch_bwd_only(ops, o, p):
    drop = ops.drop_args(SEED, CALL, p, site=R.SITE_ATTN, layer=1, stack=0)
    ops.attn_stream_bwd_drop(**o.bwd_kwargs(False), drop=drop, deterministic=True)
    torch.cuda.synchronize()
    return {n: o.b[n].t.clone() for n in ("dqkv", "dbias", "dbias_ws")}


@pytest.mark.parametrize("hd", [32, 64])
@pytest.mark.parametrize("T", [1, 17, 127, 128, 129, 257, 513])
def test_attention_pair_within_the_fp64_bound(ops, T, hd):
    B = 3
    fails = []
    for f in _forms(B, T):
        f["hd"] = hd
        fails += [f"{ar.describe(f)}: {x}" for x in _attn_case(ops, f)[4]]
    assert not fails, fails


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_pair_ragged(ops, hd):
    lens = [0, 1, 128, 129, 417]
    f = ar.fields(len(lens), max(lens), 2, hd, "ragged", seq_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    fails = _attn_case(ops, f)[4]
    assert not fails, fails


def test_attention_keep_rate(ops):
    """dV of ones-like operands cannot show the mask; the share of exactly-zero probabilities can: out with v = identity-like columns.
    q = k = 0 gives P = 1 / T exactly; with V = e_k (one-hot in the first hd keys) out[q][d] = scale / T where key d is kept, else 0."""
    B, T, H, hd, p = 16, 64, 2, 64, 0.1
    f = ar.fields(B, T, H, hd, "none")
    o = ar.Operands(f, dev(), seed=1)
    qkv = torch.zeros(o.R, 3, H, hd, dtype=torch.bfloat16, device=dev())
    qkv[:, 2] = torch.eye(T, hd, device=dev())[None].expand(B, T, hd).reshape(o.R, hd)[:, None, :].to(torch.bfloat16)
    o.view("qkv")[:] = qkv.reshape(o.R, 3 * H * hd)
    ops.attn_stream_fwd_drop(**o.fwd_kwargs(), drop=ops.drop_args(SEED, CALL, p, site=R.SITE_ATTN, layer=1, stack=0))
    torch.cuda.synchronize()
    got = (o.view("out").float().reshape(B, T, H, hd) != 0).permute(0, 2, 1, 3)               # [B][H][q][k = d]
    want = _keep_scale(B, H, T, p)
    assert torch.equal(got, want)
    assert got.numel() >= 100000 and binomial_ok(got, p)


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_pair_rejects_the_mutations(ops, hd):
    """T = 129, key mask: the launch's outputs against references built with a wrong mask or scale must fail; so must outputs in which
    the mask is missing from dqkv only.  'peaked' scores: few keys carry a row, so a wrong mask moves elements far outside the bound."""
    B, T, H, p = 3, 129, 2, 0.1
    f = _forms(B, T)[1]
    f["hd"] = hd
    o, ex_f, ex_b, (snap_f, outs_f, snap_b, outs_b), fails = _attn_case(ops, f, p, regime="peaked")
    assert not fails, fails
    sc = float(R.thr_scale(p)[1])
    right = _keep_scale(B, H, T, p).double()
    wrong = {"no scale": right, "scale twice": right * sc * sc, "mask transposed in (q, k)": _keep_scale(B, H, T, p, transpose=True).double() * sc,
             "one mask for all heads": _keep_scale(B, H, T, p, one_head=True).double() * sc,
             "another layer's mask": _keep_scale(B, H, T, p, layer=2).double() * sc,
             "another call's mask": _keep_scale(B, H, T, p, call=CALL + 1).double() * sc}
    for what, ks in wrong.items():
        mf = R.reference_fwd_drop(ar, o, ks)
        assert ar.check(o, mf, snap_f, "fwd", outs_f)[0], f"forward mutation '{what}' was not rejected"
        mb = R.reference_bwd_drop(ar, o, ex_f, ks)
        assert ar.check(o, mb, snap_b, "bwd", outs_b, folded=True)[0], f"backward mutation '{what}' was not rejected"
    # mask not applied in dqkv: the backward of the parent entry on the dropped forward's out / lse
    o.reset_outputs("bwd")
    ops.attn_stream_bwd(**o.bwd_kwargs(False))
    torch.cuda.synchronize()
    plain = {n: o.b[n].t.clone() for n in snap_b}
    assert ar.check(o, ex_b, snap_b, "bwd", plain, folded=True)[0], "a backward without the mask was not rejected"
