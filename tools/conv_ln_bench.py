#!/usr/bin/env python3
"""The four kernels of the mode="layer_norm" conv front-end in isolation at the production shapes (256 clips of 2.01 s, C = 512):
us per launch and TB/s of algorithmic bytes, cold operands (two buffer sets of 0.8-1.7 GB each: no launch finds its inputs cached),
dense forms and listed forms on a ragged-like plan (runs of 37 rows covering ~20 % of a clip), with wj_layernorm_fwd (bf16 in,
bf16 out) at the same M x D in the same process as the yardstick.

  python tools/conv_ln_bench.py            # CONV_LN_BENCH_REPS launches per line (default 10), CONV_LN_BENCH_CLIPS clips (default 256)"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavjepa_amd import ops  # noqa: E402
from wavjepa_amd.conv_frontend import conv_geometry  # noqa: E402

SPEC = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)]


def timed(label, fn, sets, reps, nbytes, note=""):
    for s in sets:
        fn(s)
    torch.cuda.synchronize()
    ev = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(sets[i % len(sets)])
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    med = us[len(us) // 2]
    print(f"{label:34s} median {med:9.1f} us  min {us[0]:9.1f}  {nbytes / med / 1e6:6.2f} TB/s ({nbytes / 1e6:.0f} MB) {note}", flush=True)


def listed_rows(n_clips, P, L, frac=0.2, run=37, seed=0):
    """ascending global rows n*P + t: runs of `run` frames covering ~frac of every clip -> (rows, row_off, max_rows)"""
    rng = np.random.default_rng(seed)
    rows, off = [], [0]
    for n in range(n_clips):
        live = np.zeros(L, bool)
        for st in rng.integers(0, max(1, L - run), max(1, int(frac * L / run))):
            live[st:st + run] = True
        t = np.nonzero(live)[0]
        rows.append(n * P + t)
        off.append(off[-1] + t.size)
    rows = np.concatenate(rows).astype(np.int32)
    return rows, np.asarray(off, np.int32), int(np.diff(off).max())


def main():
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("CONV_LN_BENCH_REPS", "10"))
    N = int(os.environ.get("CONV_LN_BENCH_CLIPS", "256"))
    n_samples, C = 32160, 512
    Ls, Ps = conv_geometry(n_samples, SPEC)
    bf, f32 = torch.bfloat16, torch.float32
    gamma, beta, bias = 1 + 0.1 * torch.randn(C, device=dev), 0.05 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)

    # ---- layer 0: N x L[0] rows from the audio
    L0, P0 = Ls[0], Ps[0]
    M0 = N * P0
    _, k0, s0 = SPEC[0]
    print(f"layer 0: {N} clips x {L0} rows (P = {P0}), C = {C}, taps = {k0}")
    w0 = (torch.randn(C, 1, k0, device=dev) * (2.0 / k0) ** 0.5).to(bf)
    sets = [dict(audio=torch.randn(N, 1, n_samples, device=dev).to(bf), act=torch.empty(M0, C, dtype=bf, device=dev),
                 dact=torch.randn(M0, C, device=dev).to(bf), mean=torch.empty(M0, device=dev), rstd=torch.empty(M0, device=dev)) for _ in range(2)]
    geo = dict(N=N, C_in=1, L=n_samples, C=C, k=k0, stride=s0, L_out=L0, P=P0)
    ws = torch.empty(ops.workspace_bytes("wj_conv0_ln_gelu_bwd", N=N, C_in=1, C=C, k=k0, L_out=L0, max_rows=0) // 4, device=dev)
    dw, dbs, dg, db = torch.zeros(C, 1, k0, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    rows, off, mx = listed_rows(N, P0, L0)
    d_rows, d_off = torch.from_numpy(np.concatenate([rows, np.zeros(256, np.int32)])).to(dev), torch.from_numpy(off).to(dev)
    live0 = N * L0
    timed("conv0_ln_fwd dense", lambda s: ops.conv0_ln_fwd(s["audio"], w0, bias, gamma, beta, s["act"], s["mean"], s["rstd"], **geo), sets, reps,
          live0 * C * 2 + N * n_samples * 2 + live0 * 8)
    timed("conv0_ln_bwd dense", lambda s: ops.conv0_ln_bwd(s["audio"], w0, bias, gamma, beta, s["mean"], s["rstd"], s["dact"], dw, dbs, dg, db, ws, **geo),
          sets, reps, live0 * C * 2 + N * n_samples * 2 + live0 * 8, "(+ partial records and two folds)")
    timed(f"conv0_ln_bwd listed {rows.size} rows", lambda s: ops.conv0_ln_bwd(s["audio"], w0, bias, gamma, beta, s["mean"], s["rstd"], s["dact"], dw,
                                                                               dbs, dg, db, ws, rows=d_rows, row_off=d_off, max_rows=mx, **geo),
          sets, reps, rows.size * (C * 2 + 8 + 2 * k0), "(+ partial records and two folds)")
    del sets, ws
    torch.cuda.empty_cache()

    # ---- layer 1: the rows the conv GEMM wrote
    L1, P1 = Ls[1], Ps[1]
    M = N * P1
    live = N * L1
    print(f"layer 1: M = {M} rows ({N} x {P1}, {L1} frames), C = {C}")
    sets = [dict(pre=torch.randn(M, C, device=dev).to(bf), post=torch.empty(M, C, dtype=bf, device=dev), dpost=torch.randn(M, C, device=dev).to(bf),
                 dpre=torch.empty(M, C, dtype=bf, device=dev), mean=torch.empty(M, device=dev), rstd=torch.empty(M, device=dev),
                 fm=torch.empty(M, device=dev), fr=torch.empty(M, device=dev)) for _ in range(2)]
    ws = torch.empty(ops.workspace_bytes("wj_layernorm_bwd", D=C) // 4, device=dev)
    rows, _, _ = listed_rows(N, P1, L1)
    d_rows = torch.from_numpy(np.concatenate([rows, np.zeros(256, np.int32)])).to(dev)
    seg = dict(M=M, C=C, seg_rows=P1, seg_valid=L1)
    timed("ln_fwd (bf16 -> bf16) yardstick", lambda s: ops.layernorm_fwd(s["pre"], gamma, beta, M=M, D=C, eps=1e-5, y_bf16=s["post"], mean=s["fm"],
                                                                         rstd=s["fr"], x_is_bf16=True), sets, reps, M * C * 4 + M * 8)
    timed("conv_ln_gelu_fwd dense", lambda s: ops.conv_ln_gelu_fwd(s["pre"], gamma, beta, s["post"], mean=s["mean"], rstd=s["rstd"], **seg), sets, reps,
          live * C * 2 + M * C * 2 + M * 8)
    timed("conv_ln_gelu_bwd dense", lambda s: ops.conv_ln_gelu_bwd(s["dpost"], s["pre"], s["mean"], s["rstd"], gamma, beta, s["dpre"], ws, **seg), sets,
          reps, live * C * 4 + M * C * 2 + live * 8, f"(partial rows {ops.conv_ln_bwd_partial_rows(M, C)})")
    timed(f"conv_ln_gelu_bwd listed {rows.size} rows", lambda s: ops.conv_ln_gelu_bwd(s["dpost"], s["pre"], s["mean"], s["rstd"], gamma, beta, s["dpre"],
                                                                                     ws, rows=d_rows, n_rows=int(rows.size), **seg), sets, reps,
          rows.size * (C * 6 + 12), f"(partial rows {ops.conv_ln_bwd_partial_rows(int(rows.size), C)})")


if __name__ == "__main__":
    main()
