"""The scene reference helper (tests/scene_reference.py) on the host.

  * its fp64 references agree with oracle/scene_oracle.py to 1e-12 relative;
  * `emulate_rir_convolve` (torch fp32 FFTs in the kernel's block / partition structure) stays at or below 0.25 of the bound on every
    GPU case and regime, and KF is the smallest power of two for which it does; its second form, which restates the pair packing as
    well, stays within the bound and keeps silent stretches exactly silent; `emulate_snr_mix` (the chunked sums in the kernels'
    order) stays below MARGIN of the bound of the gain and within the bound of the output, whose last term is ONE rounding and is
    attained.  The ratios are printed;
  * every mutation of the emulation's output is rejected wherever it applies, each applies somewhere, the unmutated output is accepted;
  * every field of the two argument structs is handled by the reference or named in its exclusion list;
  * argument errors of the two entries are answered before the device is touched.
"""
import collections
import ctypes

import numpy as np
import pytest
import torch

from oracle import scene_oracle as S
from tests import norm_reference as nr
from tests import scene_reference as sr
from wavjepa_amd import _abi

MARGIN = 0.8


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_references_agree_with_the_oracle():
    B, C, T, L = 2, 2, 1537, 1025
    c = sr.conv_inputs("decay", B, C, T, L, 1024, 1)
    ref = sr.rir_convolve(c["x"], c["h"], 1024)["y"][0]
    assert rel(ref, S.convolve_with_rir(c["x"].numpy(), c["h"].numpy())) < 1e-12
    prev = torch.randn(B, C, T, generator=torch.Generator().manual_seed(2))
    assert rel(sr.rir_convolve(c["x"], c["h"], 0, prev)["y"][0], prev.double().numpy() + S.convolve_with_rir(c["x"].numpy(), c["h"].numpy())) < 1e-12
    for seed in range(6):
        m = sr.snr_inputs("randn", 3, 2, 8191, seed)
        ref = sr.snr_mix(**m)["out"][0]
        want = S.add_noise(m["source"].numpy(), m["noise"].numpy(), m["snr"].numpy(), m["start"].numpy(), m["length"].numpy())
        assert rel(ref, want) < 1e-12


def test_convolution_emulation_sets_kf_and_mutations_are_rejected():
    w, packed = collections.defaultdict(float), collections.defaultdict(float)
    applied = collections.Counter()
    half = 0.0
    for fft, case, regime, acc in sr.conv_runs():
        B, C, T, L = case
        c = sr.conv_inputs(regime, B, C, T, L, sr.fft_n(fft), 31 + T + L, acc)
        got = t(sr.emulate_rir_convolve(c["x"], c["h"], fft, c["prev"]))
        full = sr.rir_convolve(c["x"], c["h"], fft, c["prev"])
        ref = full["y"]
        w[(sr.fft_n(fft), regime)] = max(w[(sr.fft_n(fft), regime)], nr.worst(got, *ref))
        half = max(half, nr.worst(got, ref[0], ref[1] - full["_kf_term"][0] / 2))          # the same bound at KF / 2
        nr.check(got, *ref, what=f"fft {fft} {case} {regime} accumulate={acc}")
        faithful = t(sr.emulate_rir_convolve(c["x"], c["h"], fft, c["prev"], packed=True))
        r = nr.check(faithful, *ref, what=f"packed: fft {fft} {case} {regime} accumulate={acc}")
        packed[(sr.fft_n(fft), regime)] = max(packed[(sr.fft_n(fft), regime)], r)
        silent = ref[1] == 0
        assert bool((got[silent] == ref[0][silent]).all()) and bool((faithful[silent] == ref[0][silent]).all()), \
            f"{case} {regime}: a silent stretch is not exact"
        for label, m in sr.conv_mutations(got, c["x"], c["h"], fft, c["prev"]):
            if m is None:
                continue
            applied[label] += 1
            assert nr.rejected(m, *ref), f"fft {fft} {case} {regime} accumulate={acc}: '{label}' accepted"
    print()
    for (n, regime), v in sorted(w.items()):
        print(f"emulation / bound  rir_convolve N={n:<5} {regime:8s} {v:.4f}   with the pair packing {packed[(n, regime)]:.4f}")
    worst = max(w.values())
    print(f"KF = {sr.KF}: worst {worst:.4f}; at KF / 2: {half:.4f}")
    assert worst <= sr.KF_MARGIN, f"emulation above {sr.KF_MARGIN} of the bound at KF = {sr.KF}: {worst}"
    assert half > sr.KF_MARGIN, f"KF = {sr.KF} is not the smallest power of two: half of it still leaves {half}"
    print("mutations applied:", dict(applied))
    assert len(applied) == 8 and min(applied.values()) >= 3, applied


def test_snr_emulation_stays_below_the_margin_and_mutations_are_rejected():
    w, w_out = collections.defaultdict(float), collections.defaultdict(float)
    applied = collections.Counter()
    for (B, C, T), regime, seed in sr.snr_runs():
        m = sr.snr_inputs(regime, B, C, T, seed)
        emu = sr.emulate_snr_mix(**m)
        got = t(emu["out"])
        ref = sr.snr_mix(**m)
        w[regime] = max(w[regime], nr.worst(t(emu["a"]), *ref["a"]))
        w_out[regime] = max(w_out[regime], nr.worst(got, *ref["out"]))
        nr.check(got, *ref["out"], what=f"snr_mix {(B, C, T)} {regime} seed {seed}")
        quiet = ref["a"][0] == 0
        assert torch.equal(got[quiet], m["source"][quiet]), "a = 0 must leave the source bit for bit"
        for label, mut in sr.snr_mutations(got, **m):
            if mut is None:
                continue
            applied[label] += 1
            assert nr.rejected(mut, *ref["out"]), f"snr_mix {(B, C, T)} {regime} seed {seed}: '{label}' accepted"
    print()
    for k, v in w.items():
        print(f"emulation / bound  snr_mix {k:18s} gain {v:.3f}   out {w_out[k]:.3f} (its last term is one rounding: up to 1)")
    print("mutations applied:", dict(applied))
    assert max(w.values()) < MARGIN, dict(w)
    assert len(applied) == 6 and min(applied.values()) >= 3, applied


def test_every_field_of_the_argument_structs_is_handled_or_excluded():
    for name, handled in sr.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        assert fields - handled == set(), f"{name}: fields without a reference: {sorted(fields - handled)}"
        assert handled - fields == set(), f"{name}: listed but not in the header: {sorted(handled - fields)}"
    assert set(sr.EXCLUDED) == {"wj_snr_mix_args"} and set(sr.EXCLUDED["wj_snr_mix_args"]) == {"start<0"}


def test_entries_reject_bad_arguments_without_a_gpu():
    """wj_rir_convolve and wj_snr_mix validate before they touch the device"""
    lib = _abi.load()
    ARG = -1
    a = _abi.STRUCTS["wj_rir_conv_args"]()
    assert lib.wj_rir_convolve(ctypes.byref(a), None) == ARG                      # null pointers
    a.x = a.h = a.y = a.workspace = 16
    a.B, a.C, a.T, a.L, a.h_stride_b, a.h_stride_c = 1, 2, 16, 4, 8, 4
    for field, bad in (("T", 0), ("L", 0), ("B", 0), ("C", -1), ("fft_size", 4096), ("fft_size", 512), ("h_stride_c", 3), ("h_stride_b", 7)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert lib.wj_rir_convolve(ctypes.byref(a), None) == ARG, (field, bad)
        setattr(a, field, old)
    assert _abi.workspace_bytes("wj_rir_convolve", a) == (1 * 1 * 4097 + 1 * 2 * 1 * 4097) * 8
    a.fft_size = 1024
    assert _abi.workspace_bytes("wj_rir_convolve", a) == (1 * 1 * 513 + 1 * 2 * 1 * 513) * 8
    m = _abi.STRUCTS["wj_snr_mix_args"]()
    assert lib.wj_snr_mix(ctypes.byref(m), None) == ARG
    m.source = m.noise = m.out = m.snr = m.start = m.length = m.workspace = 16
    m.B, m.C, m.T = 2, 3, 0
    assert lib.wj_snr_mix(ctypes.byref(m), None) == ARG                           # T = 0
    m.T, m.C = 5, 0
    assert lib.wj_snr_mix(ctypes.byref(m), None) == ARG
    m.C = 3
    assert _abi.workspace_bytes("wj_snr_mix", m) == 2 * 3 * 64 * 2 * 4
    for field in ("source", "noise", "out", "snr", "start", "length", "workspace"):
        setattr(m, field, 0)
        assert lib.wj_snr_mix(ctypes.byref(m), None) == ARG, field
        setattr(m, field, 16)
