"""Op-level parity of the two pre-norm LayerNorm entries (wj_layernorm_pre_fwd / wj_layernorm_pre_bwd) against fp32 torch math on
the device (GPU only), with the bounds tests/test_ops_gpu.py::test_layernorm_fwd_bwd uses for the same quantities.

bf16 outputs are compared bit for bit with the rounded f32 outputs of the same launch (y_f32 is an optional output of the forward,
ds_f32 of the backward).  Every output buffer is pre-filled with NaN and sits between guard rows: the kernels must overwrite all of
[M][D] and nothing else.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GUARD = 3      # NaN rows in front of and behind every output
EPS = 1e-6

# (1, 64) .. (9, 1024): every kernel instance of the dispatch (V = 1..4 chunks, 32 / 64 lanes per row), odd row counts, fewer rows than
# a workgroup holds; (400, 768): several workgroups; (16391, 768) / (32775, 384): 7 rows past the switch of the backward from one pass
# per wave to the capped four-pass grid (16 384 row slots; two rows per slot at D = 384)
CASES = [(1, 64), (11, 128), (67, 384), (37, 768), (9, 1024), (400, 768), (16391, 768), (32775, 384)]


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


def rnd(*shape, scale=1.0, dtype=torch.float32, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev())


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


class Guarded:
    """An [M][*] output between GUARD rows, all NaN before the launch."""
    def __init__(self, M, D=None, dtype=torch.float32):
        shape = (M + 2 * GUARD,) + ((D,) if D else ())
        self.buf = torch.full(shape, float("nan"), dtype=dtype, device=dev())
        self.view = self.buf[GUARD:GUARD + M]

    def check(self, what):
        assert bool(torch.isfinite(self.view.float()).all()), f"{what}: NaN left inside [M][D]"
        assert bool(torch.isnan(self.buf[:GUARD].float()).all()) and bool(torch.isnan(self.buf[GUARD + self.view.shape[0]:].float()).all()), \
            f"{what}: a guard row was written"
        return self.view


def bound(M, small, large):
    return small if M < 1000 else large


def fold_partials(ops, ws, rows, D, deterministic):
    """[rows][3][D] partial rows -> [3][D] sums by the library's fold: the grouped one the engine defers to (up to 2304 columns), the
    single-matrix one beyond (D = 1024)."""
    out = torch.zeros(3, D, device=dev())
    if 3 * D <= 2304:
        ops.colsum_f32_group([(ws, 3 * D, rows, 3 * D, out[0], out[1], out[2], D)], deterministic=deterministic)
    else:
        ops.colsum_f32(ws, out, M=rows, N=3 * D, ldx=3 * D, deterministic=deterministic)
    return out


@pytest.mark.parametrize("M,D", CASES)
def test_layernorm_pre_fwd(ops, M, D):
    x = rnd(M, D, seed=30) + 0.25
    r = rnd(M, D, dtype=torch.bfloat16, seed=31)
    gamma = 1 + 0.1 * rnd(D, seed=32)
    beta = 0.1 * rnd(D, seed=33)
    for with_r in (True, False):
        s_ref = x + r.float() if with_r else x.clone()
        y_ref = F.layer_norm(s_ref, (D,), gamma, beta, EPS)
        mean_ref = s_ref.mean(1)
        rstd_ref = torch.rsqrt(s_ref.var(1, unbiased=False) + EPS)
        for alias in (False, True):
            xin = Guarded(M, D)
            xin.view.copy_(x)
            s = xin if alias else Guarded(M, D)
            y, yb, mean, rstd = Guarded(M, D), Guarded(M, D, torch.bfloat16), Guarded(M), Guarded(M)
            ops.layernorm_pre_fwd(xin.view, gamma, beta, M=M, D=D, eps=EPS, r=r if with_r else None, s_f32=s.view, y_f32=y.view,
                                  y_bf16=yb.view, mean=mean.view, rstd=rstd.view)
            tag = f"r={with_r} alias={alias}"
            assert relerr(s.check("s " + tag), s_ref) < 1e-5
            assert relerr(y.check("y " + tag), y_ref) < 1e-5
            assert torch.equal(yb.check("y_bf16 " + tag), y.view.to(torch.bfloat16))
            assert relerr(mean.check("mean " + tag), mean_ref) < 1e-5 and relerr(rstd.check("rstd " + tag), rstd_ref) < 1e-5
            if not alias:
                assert torch.equal(xin.check("x " + tag), x)         # the input is read only
                if with_r:
                    full_yb = yb.view.clone()
    # every output is optional: y_bf16 alone, and the plain add (no normalised output asked for)
    yb = Guarded(M, D, torch.bfloat16)
    ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=EPS, r=r, y_bf16=yb.view)
    assert torch.equal(yb.check("y_bf16 alone"), full_yb)            # the same arithmetic whichever outputs are asked for
    s = Guarded(M, D)
    ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=EPS, r=r, s_f32=s.view)
    assert torch.equal(s.check("add only"), x + r.float())


@pytest.mark.parametrize("M,D", CASES)
def test_layernorm_pre_bwd(ops, M, D):
    s = rnd(M, D, seed=40) + 0.25
    gamma = 1 + 0.1 * rnd(D, seed=42)
    beta = 0.1 * rnd(D, seed=43)
    dres = rnd(M, D, seed=45)
    mean, rstd = torch.empty(M, device=dev()), torch.empty(M, device=dev())
    ops.layernorm_pre_fwd(s, gamma, beta, M=M, D=D, eps=EPS, mean=mean, rstd=rstd)
    rows = ops.ln_pre_bwd_partial_rows(M, D)
    assert 1 <= rows <= 1536
    for dy_bf16 in (False, True):
        dy = rnd(M, D, dtype=torch.bfloat16 if dy_bf16 else torch.float32, seed=44)
        sr = s.clone().requires_grad_(True)
        g2, b2 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        F.layer_norm(sr, (D,), g2, b2, EPS).backward(dy.float())
        for mode in ("dres", "null", "alias"):
            ds_ref = sr.grad if mode == "null" else sr.grad + dres
            ds = Guarded(M, D)
            if mode == "alias":
                ds.view.copy_(dres)
            dsb = Guarded(M, D, torch.bfloat16)
            dgamma, dbeta, dbias = (torch.zeros(D, device=dev()) for _ in range(3))
            kw = dict(M=M, D=D, dy_is_bf16=dy_bf16, dres=None if mode == "null" else (ds.view if mode == "alias" else dres))
            ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, ds_f32=ds.view, ds_bf16=dsb.view, dgamma=dgamma, dbeta=dbeta, dbias=dbias, **kw)
            tag = f"dy_bf16={dy_bf16} {mode}"
            assert relerr(ds.check("ds " + tag), ds_ref) < 2e-5, tag
            assert torch.equal(dsb.check("ds_bf16 " + tag), ds.view.to(torch.bfloat16)), tag
            assert relerr(dgamma, g2.grad) < bound(M, 2e-5, 2e-4), tag
            assert relerr(dbeta, b2.grad) < bound(M, 2e-5, 2e-4), tag
            assert relerr(dbias, dsb.view.float().sum(0)) < bound(M, 1e-5, 2e-4), tag
            if mode == "alias":
                continue         # (ds now holds the result: the forms below re-read dres)
            # form 2: per-workgroup partial rows in a workspace, folded by the entry's second kernel
            wsp = Guarded(1536 * 3, D)
            dg2, db2, dbi2 = (torch.zeros(D, device=dev()) for _ in range(3))
            ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, ds_bf16=dsb.view, dgamma=dg2, dbeta=db2, dbias=dbi2, workspace=wsp.view, **kw)
            assert relerr(dg2, dgamma) < 1e-5 and relerr(db2, dbeta) < 1e-5 and relerr(dbi2, dbias) < 1e-5, tag
            assert bool(torch.isnan(wsp.buf[:GUARD]).all()) and bool(torch.isnan(wsp.view[rows * 3:]).all()), "partials beyond their rows"
            # form 3: no gradient outputs -- the partial rows stay for wj_colsum_f32_group (atomic fold, and the ordered one twice)
            ws3 = Guarded(rows * 3, D)
            ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, ds_bf16=dsb.view, workspace=ws3.view, **kw)
            ws3.check("partial rows " + tag)
            out3 = fold_partials(ops, ws3.view, rows, D, deterministic=False)
            assert relerr(out3[0], dgamma) < 1e-5 and relerr(out3[1], dbeta) < 1e-5 and relerr(out3[2], dbias) < 1e-5, tag
            det = []
            for _ in range(2):
                ws4 = torch.full((rows * 3, D), float("nan"), device=dev())
                ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, ds_bf16=dsb.view, workspace=ws4, **kw)
                det.append(fold_partials(ops, ws4, rows, D, deterministic=True))
            assert torch.equal(det[0], det[1]), tag                   # bit-identical across two launches
            assert relerr(det[0][0], dgamma) < 1e-5 and relerr(det[0][1], dbeta) < 1e-5 and relerr(det[0][2], dbias) < 1e-5, tag
    # ds_f32 alone (the bottom of a stack) and ds_bf16 alone
    only = Guarded(M, D)
    ops.layernorm_pre_bwd(dy, s, gamma, mean, rstd, M=M, D=D, dy_is_bf16=True, dres=dres, ds_f32=only.view)
    assert relerr(only.check("ds_f32 alone"), sr.grad + dres) < 2e-5


@pytest.mark.parametrize("M,D,with_r", [(400, 768, True), (600, 384, True), (600, 384, False), (470, 768, True)])
def test_layernorm_pre_fwd_group_stats_over_the_stream(ops, M, D, with_r):
    """group_stats at group_rows = 200: per group and quarter (sum s, sum s^2) of the STREAM s = x + r, not of y; layout and quarter
    order of wj_ln_fwd_args.group_stats.  Reference: fp64 sums of the f32 s the kernel wrote, quarters added in order.  1e-6 relative;
    the inputs carry a mean so that sum(s) does not cancel (a relative bound on a sum that cancels to ~0 measures nothing).
    (470, 768): a short last group."""
    T = 200
    x = rnd(M, D, seed=50) + 0.75
    r = rnd(M, D, dtype=torch.bfloat16, seed=51) if with_r else None
    gamma = 1 + 0.1 * rnd(D, seed=52)
    beta = 0.1 * rnd(D, seed=53)
    G = -(-M // T)
    split = ops.GROUP_STATS_SPLIT
    stats = Guarded(G * split, 2)
    s, yb = Guarded(M, D), Guarded(M, D, torch.bfloat16)
    ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=EPS, r=r, s_f32=s.view, y_bf16=yb.view, group_stats=stats.view, group_rows=T)
    s_ref = x + r.float() if with_r else x
    assert torch.equal(s.check("s"), s_ref)
    assert relerr(yb.check("y").float(), F.layer_norm(s_ref, (D,), gamma, beta, EPS)) < 4e-3
    got = stats.check("group_stats").view(G, split, 2).double()
    rpp = -(-T // split)
    want = torch.zeros(G, split, 2, dtype=torch.float64, device=dev())
    for g in range(G):
        for q in range(split):
            lo, hi = g * T + q * rpp, min(M, g * T + min(T, (q + 1) * rpp))
            blk = s_ref[lo:hi].double()
            want[g, q, 0], want[g, q, 1] = blk.sum(), (blk * blk).sum()
    tot_got = torch.zeros(G, 2, dtype=torch.float64, device=dev())
    for q in range(split):             # the consumer's order
        tot_got += got[:, q]
    tot_want = want.sum(1)
    assert relerr(tot_got[:, 0], tot_want[:, 0]) < 1e-6 and relerr(tot_got[:, 1], tot_want[:, 1]) < 1e-6
    assert relerr(got, want) < 1e-6
    again = torch.empty(G * split, 2, device=dev())
    ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=EPS, r=r, y_bf16=yb.view, group_stats=again, group_rows=T)
    assert torch.equal(again, stats.view)                            # plain stores in a fixed order: bit-reproducible
    # the add-only form (the teacher's last layer) gives the same sums
    ops.layernorm_pre_fwd(x, gamma, beta, M=M, D=D, eps=EPS, r=r, s_f32=s.view, group_stats=again, group_rows=T)
    assert torch.equal(again, stats.view)
