#!/usr/bin/env python3
"""What dropout costs at the benchmark shape (base model, 256 clips of 2.01 s): ms/step of one configuration per process, and the
per-step time of the kernels the dropout launches replace or add.

    python tools/dropout_bench.py --dropout 0            # the launches of a tree without dropout
    python tools/dropout_bench.py --dropout 0.1          # student and predictor at p = 0.1
    python tools/dropout_bench.py --root OTHER_TREE      # import wavjepa_amd from another checkout (its own built library)

Run the configurations alternately from one shell script (parent tree, this tree at 0, this tree at 0.1, and again), so that clock
drift of the card lands on all alike; a configuration's figure is the median of its timed blocks over its runs.  `--profile N` then
brackets every launch of N further steps with timing events (ops.PROFILE; serialises the streams, so these are kernel times, not
step times) and prints the per-step total of each attention / LayerNorm / dropout entry.  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

CONV_SPEC = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)]
FAMILIES = ("wj_attn_fwd", "wj_attn_bwd", "wj_attn_stream_fwd_drop", "wj_attn_stream_bwd_drop", "wj_layernorm_fwd", "wj_layernorm_bwd",
            "wj_layernorm_fwd_drop", "wj_layernorm_bwd_drop", "wj_dropout_rows")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dropout", type=float, default=0.0, help="rate of the student's and the predictor's layers")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--profile", type=int, default=0, help="further steps with every launch bracketed by timing events")
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    from wavjepa_amd import ops
    from wavjepa_amd.data import SyntheticAudioSource, pinned_mask_draws
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import StepRunner
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG

    device = torch.device("cuda", 0)
    drop = dict(dropout=args.dropout) if args.dropout > 0 else {}            # (a tree without the feature refuses the argument)
    torch.manual_seed(42)
    model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                 transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(**drop),
                 transformer_decoder_cfg=TransformerEncoderCFG.create(),
                 transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384, **drop), lr=4e-4, adam_betas=(0.9, 0.98),
                 adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=2.01, nr_samples_per_audio=8, average_top_k_layers=8,
                 size="base").to(device)
    model.trainer.max_steps = 375000
    masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                    target_length=10, ratio_cutoff=0.1)
    with pinned_mask_draws(4200):
        source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=model.total_patches, seconds=10.0,
                                      seed=42, n_mask_sets=16, device=device)
    runner = StepRunner(model, gradient_clip_val=5.0)
    idx, blocks, out = 0, [], None

    def steps(n):
        nonlocal idx, out
        torch.manual_seed(1000 + idx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            out = runner.step(source.next_batch(), idx)
            idx += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    steps(args.warmup)
    for _ in range(args.blocks):
        blocks.append(steps(args.steps))
    res = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), dropout=args.dropout, clips=args.clips,
               ms_per_step=round(statistics.median(blocks), 3), ms_per_step_blocks=[round(b, 3) for b in blocks],
               final_loss=float(out["loss"].detach()))
    if args.profile > 0:
        ops.PROFILE = []
        steps(args.profile)
        per = {}
        for fn, _, e0, e1 in ops.PROFILE:
            if fn in FAMILIES:
                t, n = per.get(fn, (0.0, 0))
                per[fn] = (t + e0.elapsed_time(e1), n + 1)
        ops.PROFILE = None
        res["kernel_ms_per_step"] = {fn: round(t / args.profile, 3) for fn, (t, n) in sorted(per.items())}
        res["kernel_launches_per_step"] = {fn: n // args.profile for fn, (t, n) in sorted(per.items())}
    model._engine.wait_optimizer()
    torch.cuda.synchronize()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
