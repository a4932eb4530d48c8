"""Kernels of the mode="layer_norm" conv front-end (csrc/conv_ln.hip) through the C ABI, against an fp64 evaluation of the same bf16
inputs (GPU only).  Bounds are the yardstick forms of tests/parity_yardstick.py: the HIP result may sit ACT_FACTOR / GRAD_FACTOR times
as far from fp64 as a stock-torch restatement with the same rounding points does, plus the project's EPS.

Shapes: C in {64, 512}; 3 clips of 41 rows with 37 frames (123 rows: no multiple of the 4 / 32 rows a workgroup takes, several
workgroups); layer 0 with 10 and 20 taps, L = 815 -> 162 rows (odd per-wave share), a mono stream of a 2-channel batch through
audio_clip_stride; listed forms with a clip that has no row, the first and the last valid row, max_rows beyond every list."""
import pytest
import torch
import torch.nn.functional as F

from tests import parity_yardstick as Y

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def rnd(*shape, seed, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


rel = Y.rel
POISON = float(torch.tensor(1e4).to(torch.bfloat16))          # 1e4 as a bf16 value


def assert_act(name, hip, torch_same_rounding, f64):
    d_hip, d_ref = rel(hip, f64), rel(torch_same_rounding, f64)
    print(name, "d(HIP, fp64)", d_hip, "d(torch restatement, fp64)", d_ref)
    assert d_hip < Y.ACT_FACTOR * d_ref + Y.ACT_EPS, (name, d_hip, d_ref)


def assert_grad(name, hip, torch_same_rounding, f64):
    d_hip, d_ref = rel(hip, f64), rel(torch_same_rounding, f64)
    print(name, "d(HIP, fp64)", d_hip, "d(torch restatement, fp64)", d_ref)
    assert d_hip < Y.GRAD_FACTOR * d_ref + Y.GRAD_EPS, (name, d_hip, d_ref)


class RoundGradBf16(torch.autograd.Function):
    """identity whose gradient is rounded to bf16: the conv output's gradient is a bf16 tensor in the autocast flow"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(torch.bfloat16).to(g.dtype)


def leaf(t, dtype):
    """a fresh leaf of `dtype` (never the caller's tensor: .to() of the same dtype returns its argument)"""
    return t.detach().to(dtype).clone().requires_grad_(True)


def ln_gelu(pre, gamma, beta, dtype):
    return F.gelu(F.layer_norm(pre.to(dtype), (pre.shape[-1],), gamma.to(dtype), beta.to(dtype), 1e-5))


# ---------------------------------------------------------------------------------------------------------------- layers >= 1
NCLIP, P, L = 3, 41, 37


def valid_rows():
    return (torch.arange(NCLIP * P) % P) < L


@pytest.fixture(scope="module", params=[64, 128, 256, 512])
def layer(request, ops):
    """One draw per width, shared by the tests of the streaming kernels: inputs, the HIP forward and the three references."""
    C = request.param
    M = NCLIP * P
    pre = rnd(M, C, seed=100 + C, scale=1.5, dtype=torch.bfloat16)
    gamma, beta = 1 + 0.1 * rnd(C, seed=101), 0.05 * rnd(C, seed=102)
    dpost = rnd(M, C, seed=103, dtype=torch.bfloat16)
    ok = valid_rows().to(dev())
    dpost[~ok] = 0
    poisoned = pre.clone()
    poisoned[~ok] = float("nan")                                     # clip padding of `pre` is never read
    post = torch.full((M, C), 9.0, dtype=torch.bfloat16, device=dev())
    mean, rstd = torch.full((M,), 9.0, device=dev()), torch.full((M,), 9.0, device=dev())
    ops.conv_ln_gelu_fwd(poisoned, gamma, beta, post, M=M, C=C, mean=mean, rstd=rstd, seg_rows=P, seg_valid=L)
    refs = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        x, g, b = leaf(pre, dt), leaf(gamma, dt), leaf(beta, dt)
        y = ln_gelu(x, g, b, dt)
        y.backward(dpost.to(dt))
        dpre = x.grad * ok[:, None]
        if tag == "f32":
            dpre = dpre.to(torch.bfloat16)
            y = y.to(torch.bfloat16)
        refs[tag] = dict(post=(y.detach() * ok[:, None]), dpre=dpre, dgamma=g.grad, dbeta=b.grad, dbias=dpre.to(dt).sum(0))
    torch.cuda.synchronize()
    return dict(C=C, M=M, pre=pre, poisoned=poisoned, gamma=gamma, beta=beta, dpost=dpost, ok=ok, post=post, mean=mean, rstd=rstd, refs=refs)


def run_bwd(ops, d, dpost, pre, *, rows=None, n_rows=0, clear=False, fill=3.0, deterministic=False, fold=True):
    C, M = d["C"], d["M"]
    n = ops.conv_ln_bwd_partial_rows(n_rows if rows is not None else M, C)
    ws = torch.full((n * 3 * C + 64,), fill, device=dev())
    dpre = torch.full((M, C), 7.0, dtype=torch.bfloat16, device=dev())
    outs = [torch.zeros(C, device=dev()) for _ in range(3)] if fold else [None] * 3
    ops.conv_ln_gelu_bwd(dpost, pre, d["mean"], d["rstd"], d["gamma"], d["beta"], dpre, ws, M=M, C=C, seg_rows=P, seg_valid=L, rows=rows,
                         n_rows=n_rows, clear_dpost=clear, dgamma=outs[0], dbeta=outs[1], dbias=outs[2], deterministic=deterministic)
    torch.cuda.synchronize()
    assert bool((ws[n * 3 * C:] == fill).all())                     # nothing past the partial rows the query promised
    return dpre, outs, ws[:n * 3 * C].view(n, 3, C)


def test_conv_ln_fwd(ops, layer):
    d, r = layer, layer["refs"]
    ok = d["ok"]
    assert bool(torch.isfinite(d["post"].float()).all())
    assert float(d["post"][~ok].float().abs().max()) == 0.0           # padding rows are exact zeros
    assert_act(f"post C={d['C']}", d["post"], r["f32"]["post"], r["f64"]["post"])
    x = d["pre"].double()[ok]
    mu, var = x.mean(1), x.var(1, unbiased=False)
    assert rel(d["mean"][ok], mu) < 1e-5 and rel(d["rstd"][ok], (var + 1e-5).rsqrt()) < 1e-5
    again = torch.empty_like(d["post"])
    ops.conv_ln_gelu_fwd(d["poisoned"], d["gamma"], d["beta"], again, M=d["M"], C=d["C"], seg_rows=P, seg_valid=L)      # no statistics kept
    assert torch.equal(again.view(torch.int16), d["post"].view(torch.int16))
    nopad = torch.empty_like(d["post"])
    ops.conv_ln_gelu_fwd(d["pre"], d["gamma"], d["beta"], nopad, M=d["M"], C=d["C"])                                    # seg_rows = 0: all rows
    assert torch.equal(nopad[ok].view(torch.int16), d["post"][ok].view(torch.int16)) and float(nopad[~ok].float().abs().max()) > 0


def test_conv_ln_bwd_dense(ops, layer):
    d, r = layer, layer["refs"]
    ok = d["ok"]
    dpost = d["dpost"].clone()
    dpost[~ok] = 1e4                                                 # padding rows of dpost / pre are not read either
    dpre, (dg, db, dbi), part = run_bwd(ops, d, dpost, d["poisoned"])
    assert float(dpre[~ok].float().abs().max()) == 0.0
    assert bool((dpost[~ok].float() == POISON).all()) and torch.equal(dpost[ok], d["dpost"][ok])          # not cleared unless asked
    assert_act(f"dpre C={d['C']}", dpre, r["f32"]["dpre"], r["f64"]["dpre"])
    for name, got in (("dgamma", dg), ("dbeta", db), ("dbias", dbi)):
        assert_grad(f"{name} C={d['C']}", got, r["f32"][name], r["f64"][name])
    assert rel(dbi, dpre.double().sum(0)) < 1e-5                     # dbias = column sums of the stored bf16 dpre (fp32 sums of 111 terms)
    # workspace contents do not matter, two launches give the same bits, in both fold forms and without a fold
    dpre2, outs2, part2 = run_bwd(ops, d, dpost, d["poisoned"], fill=-5.0, deterministic=True)
    dpre3, outs3, part3 = run_bwd(ops, d, dpost, d["poisoned"], deterministic=True)
    dpre4, _, part4 = run_bwd(ops, d, dpost, d["poisoned"], fold=False)
    assert torch.equal(dpre.view(torch.int16), dpre2.view(torch.int16)) and torch.equal(dpre2.view(torch.int16), dpre4.view(torch.int16))
    assert torch.equal(part, part2) and torch.equal(part2, part3) and torch.equal(part3, part4)
    for a, b in zip(outs2, outs3):
        assert torch.equal(a, b)
    for a, b in zip(outs2, (dg, db, dbi)):
        assert rel(a, b) < 1e-5
    assert rel(part.sum(0)[0], dg) < 1e-5


def test_conv_ln_bwd_listed_rows(ops, layer):
    d = layer
    C, M, ok = d["C"], d["M"], d["ok"]
    # clip 1 has no row; the list holds the first and the last valid row of the buffer, and one padding row (written as 0, not read)
    listed = torch.tensor([0, 1, 5, 17, L - 1, L, 2 * P, 2 * P + 3, 2 * P + 20, 2 * P + L - 1], dtype=torch.int32)
    on = torch.zeros(M, dtype=torch.bool)
    on[listed.long()] = True
    on = on.to(dev())
    dense_dpre, _, _ = run_bwd(ops, d, d["dpost"], d["pre"])
    dpost = d["dpost"].clone()
    dpost[~on] = 1e4                                                 # rows off the list are never read ...
    pre = d["pre"].clone()
    pre[~on | ~ok] = float("nan")
    rows = torch.cat([listed, torch.zeros(256, dtype=torch.int32)]).to(dev())
    dpre, (dg, db, dbi), _ = run_bwd(ops, d, dpost, pre, rows=rows, n_rows=listed.numel(), clear=True)
    assert bool((dpre[~on].float() == 7.0).all())                    # ... and never written
    assert torch.equal(dpre[on].view(torch.int16), dense_dpre[on].view(torch.int16))           # the same bits as the dense form
    assert float(dpre[L].float().abs().max()) == 0.0
    assert bool((dpost[~on].float() == POISON).all()) and float(dpost[on].float().abs().max()) == 0.0      # consumed rows cleared
    # the parameter gradients are those of a dense pass over a gradient that is zero off the list
    sparse = d["dpost"] * on[:, None]
    x, g, b = leaf(d["pre"], torch.float64), leaf(d["gamma"], torch.float64), leaf(d["beta"], torch.float64)
    ln_gelu(x, g, b, torch.float64).backward(sparse.double() * ok[:, None])
    x32, g32, b32 = leaf(d["pre"], torch.float32), leaf(d["gamma"], torch.float32), leaf(d["beta"], torch.float32)
    ln_gelu(x32, g32, b32, torch.float32).backward(sparse.float() * ok[:, None])
    assert_grad("listed dgamma", dg, g32.grad, g.grad)
    assert_grad("listed dbeta", db, b32.grad, b.grad)
    assert_grad("listed dbias", dbi, x32.grad.to(torch.bfloat16).float().sum(0), x.grad.sum(0))
    # an empty list: nothing touched, zero partial rows folded
    dpre0, outs0, part0 = run_bwd(ops, d, dpost, pre, rows=rows, n_rows=0)
    assert bool((dpre0.float() == 7.0).all()) and part0.shape[0] == 1 and float(part0.abs().max()) == 0.0
    assert all(float(o.abs().max()) == 0.0 for o in outs0)


# ---------------------------------------------------------------------------------------------------------------- layer 0
N0, LA, K0, S0 = 3, 815, 10, 5
L0 = (LA - K0) // S0 + 1          # 162
P0 = 168


def conv0_refs(audio, w, bias, gamma, beta, dact):
    """audio [N, C_in, L] bf16, w [C, C_in, k] bf16 -> {tag: post [N, P0, C], dw, dbias, dgamma, dbeta} in fp64 and in the fp32 restatement
    with the kernel's rounding points (conv output bf16, straight-through; its gradient bf16; post bf16)."""
    out = {}
    for tag, dt in (("f64", torch.float64), ("f32", torch.float32)):
        wr, br = leaf(w, dt), None if bias is None else leaf(bias, dt)
        g, b = leaf(gamma, dt), leaf(beta, dt)
        y = F.conv1d(audio.to(dt), wr, br, stride=S0)
        if tag == "f32":
            y = RoundGradBf16.apply(y + (y.to(torch.bfloat16).to(dt) - y).detach())
        post = ln_gelu(y.transpose(1, 2), g, b, dt)
        post.backward(dact[:, :L0].to(dt))
        if tag == "f32":
            post = post.to(torch.bfloat16)
        full = torch.zeros(audio.shape[0], P0, w.shape[0], dtype=post.dtype, device=dev())
        full[:, :L0] = post.detach()
        out[tag] = dict(post=full, dw=wr.grad, dbias=None if br is None else br.grad, dgamma=g.grad, dbeta=b.grad)
    return out


@pytest.mark.parametrize("C,C_in,with_bias,strided", [(64, 1, True, False), (64, 2, False, False), (128, 2, True, False), (256, 1, False, True), (512, 1, False, True),
                                                        (512, 2, True, False)])
def test_conv0_ln_fwd_bwd(ops, C, C_in, with_bias, strided):
    taps = C_in * K0
    batch = rnd(N0, 2 if strided else C_in, LA, seed=200 + C + C_in, dtype=torch.bfloat16)
    ch = 1 if strided else 0
    audio = batch[:, ch:ch + 1] if strided else batch                # a mono stream of a 2-channel batch: clips 2 L apart
    geo = dict(N=N0, C_in=C_in, L=LA, C=C, k=K0, stride=S0, L_out=L0, P=P0, audio_clip_stride=2 * LA if strided else 0)
    w = rnd(C, C_in, K0, seed=201, scale=(2.0 / taps) ** 0.5, dtype=torch.bfloat16)
    bias = 0.1 * rnd(C, seed=202) if with_bias else None
    gamma, beta = 1 + 0.1 * rnd(C, seed=203), 0.05 * rnd(C, seed=204)
    dact = rnd(N0, P0, C, seed=205, dtype=torch.bfloat16)
    dact[:, L0:] = 0
    refs = conv0_refs(audio, w, bias, gamma, beta, dact)
    a_ptr = batch.data_ptr() + ch * LA * 2
    act = torch.full((N0, P0, C), 9.0, dtype=torch.bfloat16, device=dev())
    mean, rstd = torch.full((N0 * P0,), 9.0, device=dev()), torch.full((N0 * P0,), 9.0, device=dev())
    ops.conv0_ln_fwd(a_ptr, w, bias, gamma, beta, act, mean, rstd, **geo)
    torch.cuda.synchronize()
    assert float(act[:, L0:].float().abs().max()) == 0.0
    assert_act(f"conv0 post C={C} taps={taps}", act, refs["f32"]["post"], refs["f64"]["post"])
    y64 = F.conv1d(audio.double(), w.double(), None if bias is None else bias.double(), stride=S0).to(torch.bfloat16).double().transpose(1, 2)
    assert rel(mean.view(N0, P0)[:, :L0], y64.mean(2)) < 2e-3        # (the conv output is rounded to bf16 before the statistics:
    assert rel(rstd.view(N0, P0)[:, :L0], (y64.var(2, unbiased=False) + 1e-5).rsqrt()) < 2e-3   # single values may round the other way)
    act2 = torch.empty_like(act)
    ops.conv0_ln_fwd(a_ptr, w, bias, gamma, beta, act2, torch.empty_like(mean), torch.empty_like(rstd), **geo)
    assert torch.equal(act.view(torch.int16), act2.view(torch.int16))

    dims = dict(N=N0, C_in=C_in, C=C, k=K0, L_out=L0)
    ws_floats = ops.workspace_bytes("wj_conv0_ln_gelu_bwd", max_rows=0, **dims) // 4

    def bwd(dact_in, fill, **lists):
        ws = torch.full((ws_floats + 64,), fill, device=dev())
        dw, dg, db = torch.zeros(C, C_in, K0, device=dev()), torch.zeros(C, device=dev()), torch.zeros(C, device=dev())
        dbs = torch.zeros(C, device=dev()) if with_bias else None
        ops.conv0_ln_bwd(a_ptr, w, bias, gamma, beta, mean, rstd, dact_in, dw, dbs, dg, db, ws, **geo, **lists)
        torch.cuda.synchronize()
        assert bool((ws[ws_floats:] == fill).all())
        return dict(dw=dw, dbias=dbs, dgamma=dg, dbeta=db)

    poison = dact.clone()
    poison[:, L0:] = 1e4                                             # clip padding of the gradient is not read
    got = bwd(poison, 3.0)
    for name in ("dw", "dbias", "dgamma", "dbeta"):
        if got[name] is not None:
            assert_grad(f"conv0 {name} C={C} taps={taps}", got[name], refs["f32"][name], refs["f64"][name])
    again = bwd(poison, -9.0)                                        # scratch contents do not matter; the same bits twice
    assert all(torch.equal(got[k], again[k]) for k in got if got[k] is not None)

    # listed rows: clip 1 has none, the first and the last valid row are listed, max_rows is larger than every list
    live = torch.zeros(N0, L0, dtype=torch.bool)
    live[0, [0, 1, 2, 40, 41, 100]] = True
    live[2, 30:67] = True
    live[2, L0 - 1] = True
    rows = torch.nonzero(torch.cat([live, torch.zeros(N0, P0 - L0, dtype=torch.bool)], 1).reshape(-1)).squeeze(1).to(torch.int32)
    off = torch.zeros(N0 + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(live.sum(1), 0).to(torch.int32)
    sparse = torch.zeros_like(dact)
    sparse[:, :L0][live.to(dev())] = dact[:, :L0][live.to(dev())]
    refs2 = conv0_refs(audio, w, bias, gamma, beta, sparse)
    poison = sparse.clone()
    poison[:, :L0][~live.to(dev())] = 1e4                            # rows off the list are never read
    poison[:, L0:] = 1e4
    lists = dict(rows=torch.cat([rows, torch.zeros(256, dtype=torch.int32)]).to(dev()), row_off=off.to(dev()), max_rows=int(live.sum(1).max()) + 5)
    got2 = bwd(poison, 3.0, **lists)
    for name in ("dw", "dbias", "dgamma", "dbeta"):
        if got2[name] is not None:
            assert_grad(f"conv0 listed {name} C={C} taps={taps}", got2[name], refs2["f32"][name], refs2["f64"][name])
    again2 = bwd(poison, -1.0, **lists)
    assert all(torch.equal(got2[k], again2[k]) for k in got2 if got2[k] is not None)
    none = bwd(poison, 3.0, rows=lists["rows"], row_off=torch.zeros(N0 + 1, dtype=torch.int32, device=dev()), max_rows=0)
    assert all(float(v.abs().max()) == 0.0 for v in none.values() if v is not None)
