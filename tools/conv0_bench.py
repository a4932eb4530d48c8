#!/usr/bin/env python3
"""conv0 + GroupNorm + GELU forward and backward at the step's size (256 clips of 32 160 samples, 512 channels): us per launch of the
whole entry point -- the backward in its dense form and on listed rows (the ragged-like lists of tools/conv_ln_bench.py) -- and with WJ_CONV0_DUMP=<file> the activation of the first two clips (to compare the MFMA and the VALU apply pass:
WJ_CONV0_APPLY_MFMA=0/1 is read once per process).  usage: conv0_bench.py [other_dump.pt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conv_ln_bench import listed_rows  # noqa: E402
from wavjepa_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
N, C_in, L, C, k, s = 256, 1, 32160, 512, 10, 5
L_out = (L - k) // s + 1
P = (L_out + 15) // 16 * 16
g = torch.Generator(device="cpu").manual_seed(0)
audio = torch.randn(N, C_in, L, generator=g).to(torch.bfloat16).to(dev)
w = (torch.randn(C, C_in, k, generator=g) * (2.0 / (C_in * k)) ** 0.5).to(torch.bfloat16).to(dev)
gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(dev)
beta = (0.1 * torch.randn(C, generator=g)).to(dev)
act = torch.empty(N, P, C, dtype=torch.bfloat16, device=dev)
stats = torch.empty(2, N, C, device=dev)
ws = torch.empty(ops.workspace_bytes("wj_conv0_gn_gelu_fwd", N=N, C_in=C_in, C=C, k=k, L_out=L_out) // 4, device=dev)
yx, x1 = torch.empty(N, C, C_in * k, device=dev), torch.empty(N, C_in * k, device=dev)
junk = torch.empty(256 * 1024 * 1024, device=dev)


def run():
    ops.conv0_fwd(audio, w, gamma, beta, act, stats[0], stats[1], ws, N=N, C_in=C_in, L=L, C=C, k=k, stride=s, L_out=L_out, P=P, yx=yx, x1=x1)


def timed(fn):
    """sorted us of 12 launches, each after the caches were flushed"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for r in range(12):
        junk.fill_(float(r))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return sorted(ts)


ts = timed(run)
print(f"conv0 forward (stats + fold + apply) N={N}: median {ts[len(ts) // 2]:.1f} us, min {ts[0]:.1f} us; activation {act.numel() * 2 / 1e9:.2f} GB "
      f"(WJ_CONV0_APPLY_MFMA={os.environ.get('WJ_CONV0_APPLY_MFMA', '1')})")

# the backward reads the forward's mean / rstd / yx / x1 (left by the last timed launch)
dact = torch.randn(N, P, C, generator=torch.Generator(device=dev).manual_seed(1), device=dev).to(torch.bfloat16)
dact[:, L_out:] = 0
dw, dgamma, dbeta = torch.zeros(C, C_in, k, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
rows, row_off, max_rows = listed_rows(N, P, L_out)
d_rows, d_off = torch.from_numpy(np.concatenate([rows, np.zeros(256, np.int32)])).to(dev), torch.from_numpy(row_off).to(dev)
ws_b = torch.empty(ops.workspace_bytes("wj_conv0_gn_gelu_bwd", N=N, C_in=C_in, C=C, k=k, L_out=L_out, max_rows=0) // 4, device=dev)


def run_bwd(**lists):
    ops.conv0_bwd(audio, w, gamma, beta, stats[0], stats[1], dact, dw, dgamma, dbeta, ws_b, yx=yx, x1=x1, N=N, C_in=C_in, L=L, C=C, k=k, stride=s,
                  L_out=L_out, P=P, **lists)


for label, lists in (("dense", {}), (f"listed {rows.size} rows", dict(rows=d_rows, row_off=d_off, max_rows=max_rows))):
    ts = timed(lambda: run_bwd(**lists))
    print(f"conv0 backward {label} (rows + fold + finalize) N={N}: median {ts[len(ts) // 2]:.1f} us, min {ts[0]:.1f} us")
if os.environ.get("WJ_CONV0_DUMP"):
    torch.save(dict(act=act[:2].cpu(), mean=stats[0].cpu(), rstd=stats[1].cpu()), os.environ["WJ_CONV0_DUMP"])
if len(sys.argv) > 1:
    other = torch.load(sys.argv[1])
    a, b = act[:2].cpu().float(), other["act"].float()
    diff = (a != b)
    print(f"against {sys.argv[1]}: {int(diff.sum())} of {a.numel()} elements differ ({float(diff.float().mean()):.2e}), "
          f"max |diff| {float((a - b).abs().max()):.3e}, rel l2 {float((a - b).norm() / b.norm()):.3e}; "
          f"mean equal {torch.equal(stats[0].cpu(), other['mean'])}, rstd equal {torch.equal(stats[1].cpu(), other['rstd'])}")
