"""`wj_resample_fir`, `wj_mse_groups` and `wj_crop_normalize_bf16` held per element against the fp64 references and bounds of
tests/denoise_reference.py (GPU only).

Every output sits NaN-filled between guard rows; every element must come back finite and within its bound (zero bound: exactly the
reference), the guards untouched, every input bit for bit what it was, a second launch bit-identical; the grouped MSE's workspace holds
0xFF bytes before each launch.  Every mutation that applies is made on the kernel's own (accepted) output and must be rejected.

With WJ_DENOISE_BOUNDS_REPORT=<path> the module writes one line per entry and regime: the worst error / bound.
"""
import collections
import os
import time

import pytest
import torch

from tests import denoise_reference as dr
from tests import norm_reference as nr

pytestmark = pytest.mark.gpu

REPORT = collections.OrderedDict()


def note(entry, regime, ratio):
    REPORT[(entry, regime)] = max(REPORT.get((entry, regime), 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_DENOISE_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  regime  worst error / bound   (tests/test_denoise_bounds_gpu.py)\n")
            for (entry, regime), ratio in REPORT.items():
                f.write(f"{entry:24s} {regime:20s} {ratio:.3f}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------ resampler
PAIRS = sorted({(o, n) for _, _, o, n, _, _, _ in dr.resample_runs()})


@pytest.mark.parametrize("orig,nw", PAIRS)
def test_resample_fir(ops, orig, nw):
    for table, width, o, n, B, L_in, regime in dr.resample_runs():
        if (o, n) != (orig, nw):
            continue
        L_out = dr.out_len(L_in, orig, nw)
        host = dr.resample_input(regime, B, L_in, L_in + orig)
        x, k = host.to(dev()), table.to(dev())
        x0, k0 = x.clone(), k.clone()
        outs = []
        for _ in range(2):
            y = nr.Guarded(B, L_out, torch.float32, dev())
            ops.resample_fir(x, k, y.view, B=B, L_in=L_in, L_out=L_out, orig=orig, nw=nw, width=width)
            outs.append(y.check(f"resample {orig}:{nw} L_in={L_in}").cpu())
        tag = f"resample_fir {orig}:{nw} B={B} L_in={L_in} {regime}"
        assert same_bits(x, x0) and same_bits(k, k0), f"{tag}: an input was written"
        assert same_bits(outs[0], outs[1]), f"{tag}: two launches differ"
        ref = dr.resample_fir(host, table, width, orig, nw, L_out)["y"]
        note(f"resample_fir {orig}:{nw}", regime, nr.check(outs[0], *ref, what=tag))
        for label, m in dr.resample_mutations(outs[0], host, table, width, orig, nw, L_out):
            assert m is None or nr.rejected(m, *ref), f"{tag}: mutation '{label}' accepted"


def test_resample_fir_refuses_the_smallest_table_past_the_lds_limit(ops):
    """one step past the largest accepted orig : 1: WJ_ERR_UNSUPPORTED, nothing launched, y untouched"""
    from wavjepa_amd import _abi
    orig, nw, args = dr.smallest_refused_pair()
    table, width, o, n = dr.table_for(orig, nw, args)
    assert (o, n) == (orig, nw) and dr.lds_bytes(orig, nw, width) > dr.LDS_LIMIT
    L_in = 300
    L_out = dr.out_len(L_in, orig, nw)
    y = nr.Guarded(1, L_out, torch.float32, dev())
    x = dr.resample_input("randn", 1, L_in, 1).to(dev())
    with pytest.raises(_abi.WavJepaHipError, match="unsupported configuration"):
        ops.resample_fir(x, table.to(dev()), y.view, B=1, L_in=L_in, L_out=L_out, orig=orig, nw=nw, width=width)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.buf).all())


# ------------------------------------------------------------------------------------------------------------ grouped MSE
@pytest.mark.parametrize("n", dr.MSE_N)
def test_mse_groups(ops, n):
    for nn, G, regime, gscale, with_grad in dr.mse_runs():
        if nn != n:
            continue
        host = dr.mse_inputs(regime, G, n, 100 + n + G)
        p, t, w = host["preds"].to(dev()), host["targets"].to(dev()), host["w"].to(dev())
        gs = None if gscale is None else torch.tensor([gscale], device=dev())
        before = [v.clone() for v in (p, t, w)]
        nbytes = ops.workspace_bytes("wj_mse_groups", n=n, G=G)
        outs = []
        for _ in range(2):
            ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())
            loss = nr.Guarded(5, None, torch.float32, dev())
            dp = nr.Guarded(G, n, torch.float32, dev()) if with_grad else None
            ops.mse_groups(p, t, w, loss.view, ws, n=n, G=G, dpreds=None if dp is None else dp.view, gscale=gs)
            outs.append((loss.check("loss").cpu(), None if dp is None else dp.check("dpreds").cpu()))
        tag = f"mse_groups n={n} G={G} {regime} gscale={gscale} dpreds={with_grad}"
        assert all(same_bits(a, b) for a, b in zip((p, t, w), before)), f"{tag}: an input was written"
        l0, d0 = outs[0]
        assert bool(torch.isnan(l0[1 + G:]).all()), f"{tag}: loss written beyond 1 + G"
        assert same_bits(l0, outs[1][0]) and (d0 is None or same_bits(d0, outs[1][1])), f"{tag}: two launches differ"
        ref = dr.mse_groups(host["preds"], host["targets"], host["w"], gscale)
        got = {"loss": l0[:1 + G], "dpreds": d0}
        note("mse_groups loss", regime, nr.check(got["loss"], *ref["loss"], what=tag + " loss"))
        if d0 is not None:
            note("mse_groups dpreds", regime, nr.check(d0, *ref["dpreds"], what=tag + " dpreds"))
        if regime == "equal":
            assert not bool(got["loss"].any()) and (d0 is None or not bool(d0.any())), f"{tag}: preds = targets must give exact zeros"
        for label, key, m in dr.mse_mutations(got, host["preds"], host["targets"], host["w"], gscale):
            assert m is None or nr.rejected(m, *ref[key]), f"{tag}: mutation '{label}' of {key} accepted"


# ------------------------------------------------------------------------------------------------------------ crop
@pytest.mark.parametrize("B,S,C,L_full,length", dr.CROP_CASES)
def test_crop_normalize(ops, B, S, C, L_full, length):
    for b, s, c, lf, ln, regime, permute in dr.crop_runs():
        if (b, s, c, lf, ln) != (B, S, C, L_full, length):
            continue
        host = dr.crop_inputs(regime, B, S, C, L_full, length, 7 + length, permute)
        src, starts = host["src"].to(dev()), host["starts"].to(dev())
        perm_inv = None if host["perm_inv"] is None else host["perm_inv"].to(dev())
        src0, starts0 = src.clone(), starts.clone()
        outs = []
        for _ in range(2):
            out = nr.Guarded(B * S, C * length, torch.bfloat16, dev())
            ops.crop_normalize_bf16(src, starts, out.view, B=B, S=S, C=C, L_full=L_full, length=length, perm_inv=perm_inv)
            outs.append(out.check("crop out").cpu())
        tag = f"crop_normalize {(B, S, C, L_full, length)} {regime} perm={permute}"
        assert same_bits(src, src0) and same_bits(starts, starts0), f"{tag}: an input was written"
        assert same_bits(outs[0], outs[1]), f"{tag}: two launches differ"
        ref = dr.crop_normalize(host["src"], host["starts"], host["perm_inv"], length)["out"]
        note("crop_normalize_bf16", regime, nr.check(outs[0], *ref, what=tag))
        if regime == "constant":
            assert not bool(outs[0].float().any()), f"{tag}: a constant crop must come out exactly zero"
        for label, m in dr.crop_mutations(outs[0], host["src"], host["starts"], host["perm_inv"], length, regime):
            assert m is None or nr.rejected(m, *ref), f"{tag}: mutation '{label}' accepted"
