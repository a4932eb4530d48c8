"""`wj_rir_convolve` and `wj_snr_mix` held per element against the fp64 references and bounds of tests/scene_reference.py (GPU only).

Every output sits in a NaN-filled allocation between guards; every element must come back finite and within its bound (zero bound:
exactly the reference), the guards untouched, every input bit for bit what it was, a second launch bit-identical; workspaces hold
0xFF bytes before each launch.  The RIR is a channel slice of a [B][2][C][L + 5] stack whose padding and other slice are NaN.
At the end of a family's test every mutation that applies is made on the kernel's own (accepted) output and must be rejected.

With WJ_SCENE_BOUNDS_REPORT=<path> the module writes one line per entry and regime: the worst error / bound.
"""
import collections
import os
import time

import pytest
import torch

from tests import norm_reference as nr
from tests import scene_reference as sr

pytestmark = pytest.mark.gpu

REPORT = collections.OrderedDict()
MUTATED_CONV = (1024, (1, 2, 1537, 1025))
MUTATED_SNR = (3, 2, 8191)


def note(entry, regime, ratio):
    REPORT[(entry, regime)] = max(REPORT.get((entry, regime), 0.0), ratio)


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    t0 = time.time()
    yield o
    path = os.environ.get("WJ_SCENE_BOUNDS_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("# entry  regime  worst error / bound   (tests/test_scene_bounds_gpu.py)\n")
            for (entry, regime), ratio in REPORT.items():
                f.write(f"{entry:24s} {regime:20s} {ratio:.3f}\n")
            f.write(f"# wall time of the module: {time.time() - t0:.1f} s\n")


def dev():
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32)


def poisoned(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())


def flat_guarded(numel, fill=None):
    """`numel` floats between norm_reference's guard rows (GUARD rows of `numel` NaNs in front and behind)"""
    g = nr.Guarded(1, numel, torch.float32, dev())
    if fill is not None:
        g.view.copy_(fill.reshape(1, -1))
    return g


# ------------------------------------------------------------------------------------------------------------ convolution
def launch_conv(ops, fft, case, regime, acc):
    """two checked launches of one case; returns (output on the CPU, inputs, reference)"""
    B, C, T, L = case
    c = sr.conv_inputs(regime, B, C, T, L, sr.fft_n(fft), 31 + T + L, acc)
    stack = torch.full((B, 2, C, L + 5), float("nan"), device=dev())
    stack[:, 1, :, :L] = c["h"].to(dev())
    h = stack[:, 1]
    x = c["x"].to(dev())
    dims = dict(B=B, C=C, T=T, L=L, fft_size=fft)
    nbytes = ops.workspace_bytes("wj_rir_convolve", **dims)
    x0, stack0 = x.clone(), stack.clone()
    outs = []
    for _ in range(2):
        ws = poisoned(nbytes)
        y = flat_guarded(B * C * T, c["prev"])
        ops.rir_convolve(x, h, y.view, ws, h_stride_b=h.stride(0), h_stride_c=h.stride(1), accumulate=acc, **dims)
        outs.append(y.check(f"rir_convolve {case} {regime}").cpu().reshape(B, C, T))
    assert torch.equal(x, x0) and torch.equal(bits(stack), bits(stack0)), f"{case} {regime}: an input was written"
    assert torch.equal(bits(outs[0]), bits(outs[1])), f"{case} {regime}: two launches differ"
    return outs[0], c, sr.rir_convolve(c["x"], c["h"], fft, c["prev"])["y"]


@pytest.mark.parametrize("fft,case", [(fft, case) for fft, cases in sr.CONV_CASES.items() for case in cases])
def test_rir_convolve(ops, fft, case):
    for f, cs, regime, acc in sr.conv_runs():
        if (f, cs) != (fft, case):
            continue
        got, c, ref = launch_conv(ops, fft, case, regime, acc)
        tag = f"rir_convolve fft {fft} {case} {regime} accumulate={acc}"
        note(f"rir_convolve N={sr.fft_n(fft)}", regime, nr.check(got, *ref, what=tag))
        if (fft, case) == MUTATED_CONV:
            for label, m in sr.conv_mutations(got, c["x"], c["h"], fft, c["prev"]):
                assert m is None or nr.rejected(m, *ref), f"{tag}: mutation '{label}' accepted"


# ------------------------------------------------------------------------------------------------------------ SNR mix
def launch_mix(ops, m, B, C, T, out=None):
    ws = poisoned(ops.workspace_bytes("wj_snr_mix", B=B, C=C, T=T)).view(torch.float32)
    g = flat_guarded(B * C * T, out)
    dst = g.view
    ops.snr_mix(dst if out is not None else m["source"], m["noise"], dst, m["snr"], m["start"], m["length"], ws, B=B, C=C, T=T)
    return g.check("snr_mix out").cpu().reshape(B, C, T)


@pytest.mark.parametrize("case", sr.SNR_CASES)
def test_snr_mix(ops, case):
    B, C, T = case
    for cs, regime, seed in sr.snr_runs():
        if cs != case:
            continue
        host = sr.snr_inputs(regime, B, C, T, seed)
        m = {k: v.to(dev()) for k, v in host.items()}
        before = {k: v.clone() for k, v in m.items()}
        got = launch_mix(ops, m, B, C, T)
        again = launch_mix(ops, m, B, C, T)
        aliased = launch_mix(ops, m, B, C, T, out=m["source"])                 # out IS source (a copy of it inside the guards)
        for k in m:
            assert torch.equal(m[k], before[k]), f"snr_mix {case} {regime}: {k} was written"
        tag = f"snr_mix {case} {regime} seed {seed}"
        assert torch.equal(bits(got), bits(again)), f"{tag}: two launches differ"
        assert torch.equal(bits(got), bits(aliased)), f"{tag}: out aliasing source differs from the plain launch"
        ref = sr.snr_mix(**host)
        note("snr_mix", regime, nr.check(got, *ref["out"], what=tag))
        quiet = ref["a"][0] == 0
        assert torch.equal(got[quiet], host["source"][quiet]), f"{tag}: a = 0 must leave the source bit for bit"
        if case == MUTATED_SNR:
            for label, mut in sr.snr_mutations(got, **host):
                assert mut is None or nr.rejected(mut, *ref["out"]), f"{tag}: mutation '{label}' accepted"
