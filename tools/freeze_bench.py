#!/usr/bin/env python3
"""What partial training buys at the benchmark shape (WavJEPA-base, 256 clips of 2.01 s): ms/step of three frozen sets, their steps
interleaved in ONE process so that clock drift of the card lands on all alike.

    python tools/freeze_bench.py                       # rows: nothing frozen / extract_audio.* / conv stack + front + student layers 0-5
    python tools/freeze_bench.py --steps 30 --clips 64
    python tools/freeze_bench.py --root PARENT_TREE --rows nothing     # the same loop on a checkout without the feature: its step time

One model, one optimiser: the frozen set is switched between steps (JEPA.freeze / unfreeze; the engine reads it at every training
forward).  Every step is timed on its own between two device synchronisations, so no row inherits another row's overlapped optimiser
update.  Per row the median, the mean and the interquartile spread of its steps (warm-up excluded), and the box's calibration block.
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

CONV_SPEC = [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)]
ROWS = {
    "nothing": (),
    "conv": ("extract_audio.*",),
    "conv+front+enc0-5": ("extract_audio.*", "feature_norms.*", "post_extraction_mapper.*", "encoder.layers.[0-5].*"),
}


def calibration(device) -> dict:
    """What the box does on fixed work: a bf16 matmul rate and a device-to-device copy rate (medians of 5), the card's name"""
    a = torch.randn(8192, 8192, device=device, dtype=torch.bfloat16)
    buf = torch.empty(1 << 28, device=device, dtype=torch.uint8)
    out = {"device": torch.cuda.get_device_name(device)}
    for name, fn, work in (("matmul_tflops", lambda: a @ a, 2 * 8192 ** 3 / 1e12), ("copy_gbps", lambda: buf.clone(), 2 * (1 << 28) / 1e9)):
        fn()
        times = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out[name] = round(work / statistics.median(times), 1)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=4, help="untimed steps per row")
    ap.add_argument("--steps", type=int, default=24, help="timed steps per row")
    ap.add_argument("--rows", default=",".join(ROWS), help="comma-separated rows to run")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    args = ap.parse_args()
    rows_run = {r: ROWS[r] for r in args.rows.split(",")}
    switching = list(rows_run) != ["nothing"]        # (a tree without the feature is never asked to freeze)
    sys.path.insert(0, os.path.abspath(args.root))
    from wavjepa_amd.data import SyntheticAudioSource, pinned_mask_draws
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import StepRunner
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG

    device = torch.device("cuda", 0)
    cal = calibration(device)
    torch.manual_seed(42)
    model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                 transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(),
                 transformer_decoder_cfg=TransformerEncoderCFG.create(), transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384),
                 lr=4e-4, adam_betas=(0.9, 0.98), adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=2.01,
                 nr_samples_per_audio=8, average_top_k_layers=8).to(device)
    model.trainer.max_steps = 375000
    masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                    target_length=10, ratio_cutoff=0.1)
    with pinned_mask_draws(4200):
        source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=model.total_patches, seconds=10.0,
                                      seed=42, n_mask_sets=16, device=device)
    runner = StepRunner(model, gradient_clip_val=5.0)
    times = {row: [] for row in rows_run}
    idx, out = 0, None
    for it in range(args.warmup + args.steps):
        for row, patterns in rows_run.items():       # interleaved: one step of every row per round
            if switching:
                model.unfreeze("*")
            if patterns:
                model.freeze(*patterns)
            torch.manual_seed(1000 + idx)
            batch = source.next_batch()
            if model._engine is not None:
                model._engine.wait_optimizer()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = runner.step(batch, idx)
            model._engine.wait_optimizer()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[row].append((time.perf_counter() - t0) * 1e3)
            idx += 1
    rows = {}
    for row, t in times.items():
        q = statistics.quantiles(t, n=4)
        rows[row] = dict(median_ms=round(statistics.median(t), 3), mean_ms=round(statistics.fmean(t), 3), iqr_ms=round(q[2] - q[0], 3),
                         min_ms=round(min(t), 3), max_ms=round(max(t), 3), steps=len(t))
    print(json.dumps(dict(root=os.path.basename(os.path.abspath(args.root)), clips=args.clips, rows=rows, calibration=cal, final_loss=float(out["loss"].detach()))), flush=True)


if __name__ == "__main__":
    main()
