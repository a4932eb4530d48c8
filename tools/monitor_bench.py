#!/usr/bin/env python3
"""The collapse monitor's launch beside the masked-loss launch it follows, in isolation (tools/loss_bench.py's set-up): us per call of
wj_masked_moments (two kernels, with col) and of wj_masked_mse with dpreds (three kernels) at the step's shape, ragged trimmed form,
cold operands (a ring of buffer sets larger than the L2 + MALL), one process, the two entries alternated over three rounds.

  python tools/monitor_bench.py       # 512 clips x 4 groups x 200 tokens, 46601 target rows x 768
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavjepa_amd import ops  # noqa: E402

B, G, T, D, N_TGT = 512, 4, 200, 768, 46601


def main():
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("MONITOR_BENCH_REPS", "40"))
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.sort(torch.randperm(B * G * T, device=dev, generator=g)[:N_TGT]).values.to(torch.int32)
    tgt = torch.zeros(B * G * T, dtype=torch.uint8, device=dev)
    tgt[rows.long()] = 1
    n_sets = 3          # per set: 72 MB of predictions, 72 MB of dpreds, 315 MB of targets (143 MB of them on target rows)
    sets = [dict(preds=torch.randn(N_TGT, D, device=dev, generator=g).to(torch.bfloat16), targets=torch.randn(B, T, D, device=dev, generator=g),
                 dpreds=torch.empty(N_TGT, D, device=dev, dtype=torch.bfloat16)) for _ in range(n_sets)]
    loss, out = torch.zeros(2, device=dev), torch.zeros(4, device=dev)
    col = torch.zeros(2, 2, D, dtype=torch.float64, device=dev)
    ws = torch.empty(ops.workspace_bytes("wj_masked_mse", B=B, G=G, T=T) // 4, device=dev)
    mws = torch.empty(ops.workspace_bytes("wj_masked_moments", B=1, G=1, T=1, D=D, n_rows=N_TGT) // 8, dtype=torch.float64, device=dev)
    one = torch.ones(1, device=dev)
    kw = dict(B=B, G=G, T=T, D=D, rows=rows, n_rows=N_TGT)
    entries = {"wj_masked_mse + dpreds": (lambda s: ops.masked_mse(s["preds"], s["targets"], tgt, loss, ws, dpreds=s["dpreds"], gscale_ptr=one, **kw),
                                          N_TGT * D * 8 / 1e6),
               "wj_masked_moments": (lambda s: ops.masked_moments(s["preds"], s["targets"], tgt, out, mws, col=col, **kw), N_TGT * D * 6 / 1e6)}
    for rnd in range(3):
        for label, (launch, mb) in entries.items():
            for s in sets:
                launch(s)
            torch.cuda.synchronize()
            times = []
            for i in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(sets[i % n_sets])
                e1.record()
                times.append((e0, e1))
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in times)
            med = us[len(us) // 2]
            print(f"round {rnd}  {label:24s} rows={N_TGT} D={D}  median {med:7.1f} us  min {us[0]:7.1f}  {mb / med:5.2f} TB/s ({mb:.0f} MB)  "
                  f"loss {float(loss[0]):.6f}  pred_var {float(out[0]):.6f} target_var {float(out[1]):.6f} n {int(out[2])}", flush=True)


if __name__ == "__main__":
    main()
