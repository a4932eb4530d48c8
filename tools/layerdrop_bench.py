#!/usr/bin/env python3
"""What LayerDrop buys at the benchmark shape (256 clips of 2.01 s): ms/step of one configuration per process and the mean number of
layers of each stack that ran in the timed steps.

    python tools/layerdrop_bench.py                               # base model, every layer runs: the launches of a tree without LayerDrop
    python tools/layerdrop_bench.py --encoder-layerdrop 0.2       # the student's layers skipped with p = 0.2, drawn per step
    python tools/layerdrop_bench.py --size large --encoder-layerdrop 0.2
    python tools/layerdrop_bench.py --root OTHER_TREE             # import wavjepa_amd from another checkout (its own built library)

Run the configurations alternately from one shell script, so that clock drift of the card lands on all alike; a configuration's
figure is the median of its timed blocks.  A step's time follows its own kept count, so the blocks of a configuration with p > 0
differ by more than the timer's noise: `kept_enc` / `kept_dec` are the means over exactly the timed steps, and `ms_per_kept` lists
(student layers that ran, mean ms of the steps with that count), each step timed with events on the compute stream.  One JSON line."""
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
    ap.add_argument("--encoder-layerdrop", type=float, default=0.0)
    ap.add_argument("--decoder-layerdrop", type=float, default=0.0)
    ap.add_argument("--size", default="base", choices=("base", "large"))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
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
    rates = {k: v for k, v in (("encoder_layerdrop", args.encoder_layerdrop), ("decoder_layerdrop", args.decoder_layerdrop)) if v > 0}
    torch.manual_seed(42)                                                   # (a tree without the feature is never handed the keywords)
    model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                 transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(),
                 transformer_decoder_cfg=TransformerEncoderCFG.create(), transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384),
                 lr=4e-4, adam_betas=(0.9, 0.98), adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=2.01,
                 nr_samples_per_audio=8, average_top_k_layers=8, size=args.size, **rates).to(device)
    model.trainer.max_steps = 375000
    masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                    target_length=10, ratio_cutoff=0.1)
    with pinned_mask_draws(4200):
        source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=model.total_patches, seconds=10.0,
                                      seed=42, n_mask_sets=16, device=device)
    runner = StepRunner(model, gradient_clip_val=5.0)
    layers = (model.encoder.num_layers, model.decoder.num_layers)
    idx, blocks, out, kept, events = 0, [], None, [], []

    def steps(n, timed):
        nonlocal idx, out
        torch.manual_seed(1000 + idx)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            if timed:
                events.append([torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)])
                events[-1][0].record()
            out = runner.step(source.next_batch(), idx)
            idx += 1
            if timed:
                events[-1][1].record()
                last = getattr(model, "last_kept", None)
                kept.append(layers if last is None else (len(last["enc"]), len(last["dec"])))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    steps(args.warmup, False)
    for _ in range(args.blocks):
        blocks.append(steps(args.steps, True))
    per = {}
    for (e0, e1), (ke, _) in zip(events, kept):
        per.setdefault(ke, []).append(e0.elapsed_time(e1))
    res = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), size=args.size, encoder_layerdrop=args.encoder_layerdrop,
               decoder_layerdrop=args.decoder_layerdrop, clips=args.clips, layers=list(layers),
               ms_per_step=round(statistics.median(blocks), 3), ms_per_step_mean=round(statistics.fmean(blocks), 3),
               ms_per_step_blocks=[round(b, 3) for b in blocks],
               kept_enc=round(statistics.fmean(k[0] for k in kept), 3), kept_dec=round(statistics.fmean(k[1] for k in kept), 3),
               ms_per_kept=[[ke, round(statistics.fmean(v), 3), len(v)] for ke, v in sorted(per.items())],
               final_loss=float(out["loss"].detach()))
    model._engine.wait_optimizer()
    torch.cuda.synchronize()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
