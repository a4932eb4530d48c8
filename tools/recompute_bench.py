#!/usr/bin/env python3
"""Activation recomputation (JEPA use_gradient_checkpointing) at a shape given on the command line: peak HBM and ms/step with the flag
off and on, in one process.

    python tools/recompute_bench.py                               # the benchmark shape: base model, 256 clips of 2.01 s
    python tools/recompute_bench.py --seconds 10 --clips 128      # 999 tokens per clip

Both models (same seed, same batches) are built and warmed up, then timed in interleaved blocks -- off, on, off, on, ... -- so that
clock drift of the card lands on both alike; a mode's figure is the median of its blocks.  `--sequential` instead runs one mode to
the end and frees it before the other is built, for shapes at which the two arenas do not fit the card together.

Peak HBM of a mode = the highest torch.cuda.max_memory_allocated over its warm-up and blocks, less what the OTHER model holds at
that time (its parameters, optimiser state and arena are static while it does not step).  One JSON line per mode, then one with the
ratios."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_SPEC = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)]


def build(device, seconds: float, size: str, recompute: bool, norm_first: bool):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    torch.manual_seed(42)
    model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                 transformer_encoder_cfg=TransformerEncoderCFG.create(),
                 transformer_encoder_layers_cfg=TransformerLayerCFG.create(norm_first=norm_first),
                 transformer_decoder_cfg=TransformerEncoderCFG.create(),
                 transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384, norm_first=norm_first), lr=4e-4,
                 adam_betas=(0.9, 0.98), adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=seconds,
                 nr_samples_per_audio=8, average_top_k_layers=8, size=size, use_gradient_checkpointing=recompute).to(device)
    model.trainer.max_steps = 375000
    return model


class Mode:
    """One model with its runner and its own copy of the batch stream."""

    def __init__(self, args, device, recompute: bool):
        from wavjepa_amd.data import SyntheticAudioSource, pinned_mask_draws
        from wavjepa_amd.masking import TimeInverseBlockMasker
        from wavjepa_amd.trainer import StepRunner
        self.name = "on" if recompute else "off"
        before = torch.cuda.memory_allocated(device)
        self.model = build(device, args.seconds, args.size, recompute, args.norm_first)
        masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                        target_length=10, ratio_cutoff=0.1)
        with pinned_mask_draws(4200):      # the same mask sets for both modes
            self.source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=self.model.total_patches,
                                               seconds=max(10.0, args.seconds), seed=42, n_mask_sets=16, device=device)
        self.runner = StepRunner(self.model, gradient_clip_val=5.0)
        self.device, self.idx, self.blocks, self.peak, self.loss = device, 0, [], 0, float("nan")
        self.held_before = before          # what was allocated when this mode was created (the other model, if it exists)
        self.footprint = 0

    def steps(self, n: int, other_held: int, timed: bool) -> None:
        torch.manual_seed(1000 + self.idx)                 # the crop draws of the step: the same in both modes
        torch.cuda.manual_seed(1000 + self.idx)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(self.device)
        t0 = time.perf_counter()
        for _ in range(n):
            out = self.runner.step(self.source.next_batch(), self.idx)
            self.idx += 1
        torch.cuda.synchronize()
        if timed:
            self.blocks.append((time.perf_counter() - t0) * 1e3 / n)
        self.loss = float(out["loss"].detach())
        self.peak = max(self.peak, torch.cuda.max_memory_allocated(self.device) - other_held)

    def result(self, args) -> dict:
        eng = self.model._engine
        return dict(mode=self.name, recompute=eng.recompute, clips=args.clips, seconds=args.seconds, tokens=self.model.total_patches,
                    size=args.size, norm_first=args.norm_first, ms_per_step=round(statistics.median(self.blocks), 3),
                    ms_per_step_blocks=[round(b, 3) for b in self.blocks], peak_hbm_gb=round(self.peak / 1e9, 2),
                    rows_student=eng.cap_enc, rows_predictor=eng.cap_dec, final_loss=self.loss)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=256, help="clips per step (a multiple of 8: 8 crops per source audio)")
    ap.add_argument("--seconds", type=float, default=2.01, help="seconds per clip (2.01 -> 200 tokens, 10 -> 999)")
    ap.add_argument("--size", default="base", choices=("tiny", "base", "large"))
    ap.add_argument("--norm-first", action="store_true", help="pre-norm stacks")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--blocks", type=int, default=3, help="timed blocks per mode")
    ap.add_argument("--modes", default="off,on", help="off,on | off | on")
    ap.add_argument("--sequential", action="store_true", help="one mode at a time (the two arenas never share the card)")
    args = ap.parse_args()
    if args.clips % 8 or args.clips < 8:
        raise SystemExit("--clips must be a positive multiple of 8")
    names = [m.strip() for m in args.modes.split(",") if m.strip()]
    if not names or any(m not in ("off", "on") for m in names):
        raise SystemExit("--modes: off, on or off,on")
    device = torch.device("cuda", 0)
    results = {}
    if args.sequential or len(names) == 1:
        for name in names:
            mode = Mode(args, device, name == "on")
            mode.steps(args.warmup, mode.held_before, timed=False)
            for _ in range(args.blocks):
                mode.steps(args.steps, mode.held_before, timed=True)
            results[name] = mode.result(args)
            print(json.dumps(results[name]), flush=True)
            mode.model._engine.wait_optimizer()
            torch.cuda.synchronize()
            del mode
            gc.collect()
            torch.cuda.empty_cache()
    else:
        modes = []
        for name in names:
            mode = Mode(args, device, name == "on")
            mode.steps(args.warmup, mode.held_before, timed=False)
            mode.footprint = torch.cuda.memory_allocated(device) - mode.held_before
            modes.append(mode)
        for _ in range(args.blocks):
            for mode, other in ((modes[0], modes[1]), (modes[1], modes[0])):
                mode.steps(args.steps, other.footprint, timed=True)
        for mode in modes:
            results[mode.name] = mode.result(args)
            print(json.dumps(results[mode.name]), flush=True)
    if len(results) == 2:
        off, on = results["off"], results["on"]
        print(json.dumps(dict(interleaved=not args.sequential, time_ratio_on_over_off=round(on["ms_per_step"] / off["ms_per_step"], 4),
                              peak_ratio_on_over_off=round(on["peak_hbm_gb"] / off["peak_hbm_gb"], 4),
                              final_loss_off=off["final_loss"], final_loss_on=on["final_loss"])), flush=True)


if __name__ == "__main__":
    main()
