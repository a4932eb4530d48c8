#!/usr/bin/env python3
"""The masked-loss launch of the step in isolation: wj_masked_mse and every kind of wj_masked_loss, us per launch (count + rows + final
kernels) and TB/s of algorithmic bytes (2 + 4 in, 2 out per element of a target row), cold operands (a ring of buffer sets larger than
the L2 + MALL so that no launch finds its inputs cached), one process.

  python tools/loss_bench.py          # the step's shape: 512 clips x 4 groups x 200 tokens, 46601 target rows x 768, ragged, with dpreds
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavjepa_amd import ops  # noqa: E402

B, G, T, D, N_TGT = 512, 4, 200, 768, 46601
KINDS = [("wj_masked_mse", None, 1.0), ("mse", "mse", 1.0), ("l1", "l1", 1.0), ("smooth_l1 beta=1", "smooth_l1", 1.0),
         ("smooth_l1 beta=0.25", "smooth_l1", 0.25), ("huber delta=1", "huber", 1.0)]


def main():
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("LOSS_BENCH_REPS", "40"))
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.sort(torch.randperm(B * G * T, device=dev, generator=g)[:N_TGT]).values.to(torch.int32)
    tgt = torch.zeros(B * G * T, dtype=torch.uint8, device=dev)
    tgt[rows.long()] = 1
    n_sets = 3          # per set: 72 MB of predictions, 72 MB of dpreds, 315 MB of targets (143 MB of them on target rows)
    sets = [dict(preds=torch.randn(N_TGT, D, device=dev, generator=g).to(torch.bfloat16), targets=torch.randn(B, T, D, device=dev, generator=g),
                 dpreds=torch.empty(N_TGT, D, device=dev, dtype=torch.bfloat16)) for _ in range(n_sets)]
    loss = torch.zeros(2, device=dev)
    ws = torch.empty(ops.workspace_bytes("wj_masked_loss", B=B, G=G, T=T) // 4, device=dev)
    one = torch.ones(1, device=dev)
    mb = N_TGT * D * 8 / 1e6

    def launch(s, kind, beta):
        kw = dict(B=B, G=G, T=T, D=D, dpreds=s["dpreds"], gscale_ptr=one, rows=rows, n_rows=N_TGT)
        if kind is None:
            ops.masked_mse(s["preds"], s["targets"], tgt, loss, ws, **kw)
        else:
            ops.masked_loss(s["preds"], s["targets"], tgt, loss, ws, kind=kind, beta=beta, **kw)

    for rnd in range(2):            # every entry twice, in order: the spread between the two rounds is the run-to-run noise of this process
        for label, kind, beta in KINDS:
            for s in sets:
                launch(s, kind, beta)
            torch.cuda.synchronize()
            times = []
            for i in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                launch(sets[i % n_sets], kind, beta)
                e1.record()
                times.append((e0, e1))
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in times)
            med = us[len(us) // 2]
            print(f"round {rnd}  {label:20s} rows={N_TGT} D={D}  median {med:7.1f} us  min {us[0]:7.1f}  {mb / med:5.2f} TB/s ({mb:.0f} MB)  "
                  f"loss {float(loss[0]):.6f} count {int(loss[1])}", flush=True)


if __name__ == "__main__":
    main()
