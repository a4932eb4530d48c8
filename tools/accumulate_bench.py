#!/usr/bin/env python3
"""What gradient accumulation costs at the benchmark shape (base model, 2.01 s clips): one configuration per process.

    python tools/accumulate_bench.py --clips 256                 # k = 1: the step as it always was
    python tools/accumulate_bench.py --clips 64 --k 4            # four micro-batches of 64 clips per optimiser step
    python tools/accumulate_bench.py --root OTHER_TREE           # import wavjepa_amd from another checkout (its own built library)

Run the configurations alternately from one shell script (parent tree at k = 1, this tree at k = 1, this tree at k = 4, and again), so
that clock drift of the card lands on all alike; a configuration's figure is the median of its timed blocks over its runs.  At k > 1 a
further pass brackets every call of StepRunner.step with timing events and reports the median of the non-closing and of the closing
micro-batches (the events add a few microseconds per call; the block times above are taken without them).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

CONV_SPEC = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)]


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--k", type=int, default=1, help="accumulate_grad_batches (1: the argument is not passed at all)")
    ap.add_argument("--clips", type=int, default=256, help="clips per micro-batch")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    ap.add_argument("--warmup", type=int, default=5, help="optimiser steps before the first timed block")
    ap.add_argument("--steps", type=int, default=10, help="optimiser steps per timed block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from wavjepa_amd.data import SyntheticAudioSource, pinned_mask_draws
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import StepRunner
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG

    device = torch.device("cuda", 0)
    torch.manual_seed(42)
    model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                 transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(),
                 transformer_decoder_cfg=TransformerEncoderCFG.create(),
                 transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384), lr=4e-4, adam_betas=(0.9, 0.98),
                 adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=2.01, nr_samples_per_audio=8, average_top_k_layers=8,
                 size="base").to(device)
    model.trainer.max_steps = 375000
    masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                    target_length=10, ratio_cutoff=0.1)
    with pinned_mask_draws(4200):
        source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=model.total_patches, seconds=10.0,
                                      seed=42, n_mask_sets=16, device=device)
    k = args.k
    kw = dict(accumulate_grad_batches=k) if k > 1 else {}               # (a tree without the feature refuses the argument)
    runner = StepRunner(model, gradient_clip_val=5.0, **kw)
    idx, blocks, out = 0, [], None

    def steps(n, events=None):
        """n optimiser steps = n * k calls -> ms per optimiser step (host clock, synchronised at both ends)"""
        nonlocal idx, out
        torch.manual_seed(1000 + idx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n * k):
            if events is not None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            out = runner.step(source.next_batch(), idx)
            if events is not None:
                e1.record()
                events.append((idx % k == k - 1, e0, e1))
            idx += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    steps(args.warmup)
    for _ in range(args.blocks):
        blocks.append(steps(args.steps))
    res = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), k=k, clips_per_micro_batch=args.clips, clips_per_step=args.clips * k,
               ms_per_optimiser_step=round(statistics.median(blocks), 3), ms_per_optimiser_step_blocks=[round(b, 3) for b in blocks])
    if k > 1:
        events = []
        steps(args.steps, events)
        for closing, name in ((False, "ms_per_non_closing_micro_batch"), (True, "ms_per_closing_micro_batch")):
            res[name] = round(statistics.median(a.elapsed_time(b) for c, a, b in events if c == closing), 3)
    model._engine.wait_optimizer()
    torch.cuda.synchronize()
    res["max_memory_allocated_gib"] = round(torch.cuda.max_memory_allocated(device) / 2**30, 3)
    res["final_loss"] = float(out["loss"].detach())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
