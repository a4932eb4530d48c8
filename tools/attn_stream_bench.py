#!/usr/bin/env python3
"""The block-streamed attention launches in isolation: us per launch and achieved TFLOP/s, cold operands (a ring of three operand sets of
0.9-3.1 GB each, far above L2 + MALL, so that no launch finds its inputs cached), median of ATTN_BENCH_REPS (default 30) event-timed
launches after a warm-up pass over every set.

  python tools/attn_stream_bench.py            # 256 clips x 12 heads x 64: wj_attn_stream_fwd / _bwd at T = 400, 499, 1000 and, as the
                                               # yardstick in the same process, wj_attn_fwd / wj_attn_bwd at T = 400 (the only shape both run)

TFLOP/s counts the ALGORITHM's operations -- forward 4 T^2 hd per (clip, head) (Q K^T and P V), backward 10 T^2 hd (S, dP, dV, dQ, dK) --
not the kernels' recomputation (the streamed forward takes Q K^T twice, both backwards take S and dP twice), so the figures of the two
families compare as time does.  Dense form, no mask, lse stored, dbias with the fold left to the caller (defer_fold), as the engine
launches the teacher / a dense stack."""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wavjepa_amd import ops  # noqa: E402

B, H, HD = 256, 12, 64
CASES = [("whole-image", 400, ops.attn_fwd, ops.attn_bwd), ("streamed", 400, ops.attn_stream_fwd, ops.attn_stream_bwd),
         ("streamed", 499, ops.attn_stream_fwd, ops.attn_stream_bwd), ("streamed", 1000, ops.attn_stream_fwd, ops.attn_stream_bwd)]


def main():
    ops.require_gpu()
    dev = torch.device("cuda", 0)
    reps = int(os.environ.get("ATTN_BENCH_REPS", "30"))
    D = H * HD
    print(f"attention launches, {B} clips x {H} heads x {HD}, bf16, dense, cold operands, median of {reps}", flush=True)
    for family, T, fwd_fn, bwd_fn in CASES:
        M = B * T
        sets = []
        for i in range(3):
            g = torch.Generator(device=dev).manual_seed(i)
            sets.append(dict(qkv=torch.randn(M, 3 * D, device=dev, generator=g).to(torch.bfloat16),
                             dout=torch.randn(M, D, device=dev, generator=g).to(torch.bfloat16),
                             out=torch.empty(M, D, device=dev, dtype=torch.bfloat16), lse=torch.empty(B * H * T, device=dev),
                             dqkv=torch.empty(M, 3 * D, device=dev, dtype=torch.bfloat16)))
        dbias = torch.zeros(3 * D, device=dev)
        ws = torch.empty(B * 3 * D, device=dev)

        def fwd(s):
            fwd_fn(s["qkv"], s["out"], B=B, T=T, H=H, hd=HD, lse=s["lse"])

        def bwd(s):
            bwd_fn(s["qkv"], s["out"], s["dout"], s["lse"], s["dqkv"], B=B, T=T, H=H, hd=HD, dbias=dbias, dbias_ws=ws, defer_fold=True)

        for label, fn, flops in (("fwd", fwd, 4.0 * T * T * HD * B * H), ("bwd", bwd, 10.0 * T * T * HD * B * H)):
            for s in sets:
                fwd(s)
                fn(s)
            torch.cuda.synchronize()
            times = []
            for i in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(sets[i % len(sets)])
                e1.record()
                times.append((e0, e1))
            torch.cuda.synchronize()
            us = sorted(a.elapsed_time(b) * 1e3 for a, b in times)
            med = us[len(us) // 2]
            print(f"{family:11s} {label} T={T:4d}  median {med:8.1f} us  min {us[0]:8.1f}  max {us[-1]:8.1f}  {flops / med / 1e6:6.1f} TFLOP/s "
                  f"({flops / 1e9:.1f} GFLOP)", flush=True)
        del sets
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
