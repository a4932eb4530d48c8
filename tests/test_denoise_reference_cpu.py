"""The resampler / grouped-MSE / crop reference helper (tests/denoise_reference.py) on the host.

  * its fp64 references agree with oracle/resample_oracle.py's application step, with torch.nn.functional.mse_loss and autograd in fp64,
    and with the crop fixture of tests/golden;
  * fp32 emulations in the kernels' documented order (the serial-fmaf FIR, the 1024 partials and their serial fold, the two-pass crop
    statistics) stay below MARGIN of every bound on every GPU case; the ratios are printed;
  * every mutation of the emulation's output is rejected wherever it applies, each applies somewhere, the unmutated output is accepted;
  * every field of the three argument structs is handled by the reference;
  * argument errors of the three entries are answered before the device is touched.
"""
import collections
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resample_oracle as RS
from tests import denoise_reference as dr
from tests import norm_reference as nr
from wavjepa_amd import _abi

MARGIN = 0.8


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_references_agree_with_oracle_torch_and_fixture(golden_dir):
    # the application step of the oracle, with the oracle's own fp64 table handed to the reference
    for fo, fn, lw, method in ((32000, 16000, 64, "sinc_interp_kaiser"), (48000, 32000, 6, "sinc_interp_hann")):
        k, width, orig, nw = RS.kernel(fo, fn, lw, 0.9475937167399596 if lw == 64 else 0.99, method)
        x = torch.randn(2, 1501, generator=torch.Generator().manual_seed(1))
        want = RS.resample(x.numpy(), fo, fn, lw, 0.9475937167399596 if lw == 64 else 0.99, method)
        ref = dr.resample_fir(x, t(k), width, orig, nw, want.shape[-1])["y"][0]
        assert rel(ref, want) < 1e-12
    # grouped MSE against F.mse_loss and autograd
    c = dr.mse_inputs("randn", 4, 1025, 2)
    p = c["preds"].double().requires_grad_(True)
    per = torch.stack([F.mse_loss(p[g], c["targets"].double()) for g in range(4)])
    loss = (c["w"].double() * per).sum()
    (loss * float(np.float32(2.5))).backward()
    ref = dr.mse_groups(c["preds"], c["targets"], c["w"], 2.5)
    assert rel(ref["loss"][0][0], loss.detach()) < 1e-12 and rel(ref["loss"][0][1:], per.detach()) < 1e-12
    assert rel(ref["dpreds"][0], p.grad) < 1e-12
    # the crop fixture: the reference's own output bits
    fx = dict(np.load(os.path.join(golden_dir, "crops.npz")))
    perm = torch.from_numpy(fx["perm"])
    perm_inv = torch.empty_like(perm)
    perm_inv[perm] = torch.arange(perm.numel())
    src = torch.from_numpy(fx["src"])
    src = src if src.dim() == 3 else src[:, None]
    L = int(fx["target_length"])
    ref = dr.crop_normalize(src, torch.from_numpy(fx["starts"]), perm_inv.to(torch.int32), L)["out"]
    want = torch.from_numpy(fx["out_bits"]).view(torch.bfloat16).reshape(ref[0].shape)
    nr.check(want, *ref, what="crop fixture")                     # the fixture is an fp32 computation: within the bound of one
    assert float((want.double() != ref[0]).double().mean()) < 2e-3


def test_resampler_emulation_margin_and_mutations():
    w = collections.defaultdict(float)
    applied = collections.Counter()
    for table, width, orig, nw, B, L_in, regime in dr.resample_runs():
        L_out = dr.out_len(L_in, orig, nw)
        x = dr.resample_input(regime, B, L_in, L_in + orig)
        got = t(dr.emulate_resample_fir(x, table, width, orig, nw, L_out))
        ref = dr.resample_fir(x, table, width, orig, nw, L_out)["y"]
        key = f"{orig}:{nw} {regime}"
        w[key] = max(w[key], nr.check(got, *ref, what=f"resample {orig}:{nw} L_in={L_in} {regime}"))
        if regime == "zero":
            assert not bool(got.any()) and not bool(ref[1].any())
        for label, m in dr.resample_mutations(got, x, table, width, orig, nw, L_out):
            if m is None:
                continue
            applied[label] += 1
            assert nr.rejected(m, *ref), f"resample {orig}:{nw} L_in={L_in} {regime}: '{label}' accepted"
    print()
    for k, v in w.items():
        print(f"emulation / bound  resample_fir {k:16s} {v:.3f}")
    print("mutations applied:", dict(applied))
    assert max(w.values()) < MARGIN
    assert len(applied) == 4 and min(applied.values()) >= 10, applied


def test_mse_emulation_margin_and_mutations():
    w = collections.defaultdict(float)
    applied = collections.Counter()
    for n, G, regime, gscale, _ in dr.mse_runs():
        c = dr.mse_inputs(regime, G, n, 100 + n + G)
        emu = dr.emulate_mse_groups(c["preds"], c["targets"], c["w"], gscale)
        got = {"loss": t(emu["loss"]), "dpreds": t(emu["dpreds"])}
        ref = dr.mse_groups(c["preds"], c["targets"], c["w"], gscale)
        for key in ("loss", "dpreds"):
            r = nr.check(got[key], *ref[key], what=f"mse_groups n={n} G={G} {regime} {key}")
            w[f"{key} {regime}"] = max(w[f"{key} {regime}"], r)
        if regime == "equal":
            assert not bool(got["loss"].any()) and not bool(got["dpreds"].any())
        for label, key, m in dr.mse_mutations(got, c["preds"], c["targets"], c["w"], gscale):
            if m is None:
                continue
            applied[label] += 1
            assert nr.rejected(m, *ref[key]), f"mse_groups n={n} G={G} {regime}: '{label}' ({key}) accepted"
    print()
    for k, v in w.items():
        print(f"emulation / bound  mse_groups {k:16s} {v:.3f}")
    print("mutations applied:", dict(applied))
    assert max(w.values()) < MARGIN
    assert len(applied) == 5 and min(applied.values()) >= 6, applied


def test_crop_emulation_margin_and_mutations():
    w = collections.defaultdict(float)
    applied = collections.Counter()
    for B, S, C, L_full, length, regime, permute in dr.crop_runs():
        c = dr.crop_inputs(regime, B, S, C, L_full, length, 7 + length, permute)
        emu = dr.emulate_crop_normalize(c["src"], c["starts"], c["perm_inv"], length)
        ref = dr.crop_normalize(c["src"], c["starts"], c["perm_inv"], length)
        tag = f"crop {(B, S, C, L_full, length)} {regime}"
        w[f"y {regime}"] = max(w[f"y {regime}"], nr.check(t(emu["y"]), *ref["y"], what=tag + " y"))
        w[f"out {regime}"] = max(w[f"out {regime}"], nr.check(t(emu["out"]), *ref["out"], what=tag + " out"))
        if regime == "constant":
            assert not emu["out"].any()
        for label, m in dr.crop_mutations(t(emu["out"]), c["src"], c["starts"], c["perm_inv"], length, regime):
            if m is None:
                continue
            applied[label] += 1
            assert nr.rejected(m, *ref["out"]), f"{tag}: '{label}' accepted"
    print()
    for k, v in w.items():
        print(f"emulation / bound  crop_normalize {k:14s} {v:.3f}")
    print("mutations applied:", dict(applied))
    assert max(v for k, v in w.items() if k.startswith("y ")) < MARGIN          # `out` adds the bf16 rounding itself: up to 1 by construction
    assert len(applied) == 6 and min(applied.values()) >= 1, applied


def test_every_field_of_the_argument_structs_is_handled():
    for name, handled in dr.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        assert fields - handled == set(), f"{name}: fields without a reference: {sorted(fields - handled)}"
        assert handled - fields == set(), f"{name}: listed but not in the header: {sorted(handled - fields)}"
    assert dr.EXCLUDED == {}


def test_entries_reject_bad_arguments_without_a_gpu():
    lib = _abi.load()
    ARG, UNSUPPORTED = -1, -3
    a = _abi.STRUCTS["wj_resample_args"]()
    assert lib.wj_resample_fir(ctypes.byref(a), None) == ARG
    a.x = a.y = a.kernel = 16
    a.B, a.L_in, a.L_out, a.orig, a.nw, a.width, a.taps = 1, 10, 5, 2, 1, 136, 274
    for field, bad in (("B", 0), ("L_in", 0), ("L_out", 0), ("orig", 0), ("nw", 0), ("width", -1), ("taps", 273)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert lib.wj_resample_fir(ctypes.byref(a), None) == ARG, (field, bad)
        setattr(a, field, old)
    orig, nw, _ = dr.smallest_refused_pair()
    width = -(-6 * orig * 100 // 99)
    assert dr.lds_bytes(orig, nw, width) > dr.LDS_LIMIT >= dr.lds_bytes(orig - 1, nw, -(-6 * (orig - 1) * 100 // 99))
    a.orig, a.nw, a.width, a.taps = orig, nw, width, 2 * width + orig
    assert lib.wj_resample_fir(ctypes.byref(a), None) == UNSUPPORTED               # refused before any launch
    _, lw, lo, ln = dr.table_for(*dr.LDS_PAIR)
    assert 48 * 1024 < dr.lds_bytes(lo, ln, lw) <= dr.LDS_LIMIT                    # the table the GPU test runs above 48 KB
    m = _abi.STRUCTS["wj_mse_groups_args"]()
    assert lib.wj_mse_groups(ctypes.byref(m), None) == ARG
    m.preds = m.targets = m.w = m.loss = m.workspace = 16
    m.n, m.G = 8, 2
    for field, bad in (("G", 0), ("G", 5), ("n", 0), ("preds", 0), ("targets", 0), ("loss", 0), ("workspace", 0)):
        old = getattr(m, field)
        setattr(m, field, bad)
        assert lib.wj_mse_groups(ctypes.byref(m), None) == ARG, (field, bad)
        setattr(m, field, old)
    assert _abi.workspace_bytes("wj_mse_groups", m) == 2 * 1024 * 4
    c = _abi.STRUCTS["wj_crop_args"]()
    assert lib.wj_crop_normalize_bf16(ctypes.byref(c), None) == ARG
    c.src = c.starts = c.out = 16
    c.B, c.S, c.C, c.L_full, c.length = 1, 1, 1, 8, 4
    for field, bad in (("B", 0), ("S", 0), ("C", 0), ("length", 1), ("L_full", 3), ("src", 0), ("starts", 0), ("out", 0)):
        old = getattr(c, field)
        setattr(c, field, bad)
        assert lib.wj_crop_normalize_bf16(ctypes.byref(c), None) == ARG, (field, bad)
        setattr(c, field, old)
