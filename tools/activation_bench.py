#!/usr/bin/env python3
"""What the feed-forward activation costs at the benchmark shape (base model, 256 clips of 2.01 s): ms/step of the four kinds, alternated
in ONE process so that clock drift of the card lands on all alike, and the per-launch time of linear1's forward GEMM at the teacher's,
the student's and the predictor's shape for each kind.

    python tools/activation_bench.py                          # gelu, relu, gelu_tanh, silu: --rounds timed blocks each, interleaved
    python tools/activation_bench.py --kinds gelu --root OTHER_TREE     # import wavjepa_amd from another checkout (its own built library)

A kind's step time is the median of its timed blocks.  `--profile N` then brackets every launch of N further steps per kind with timing
events (ops.PROFILE; serialises the streams, so these are kernel times, not step times) and reports linear1's launches (N = 4 K, one
of the two forward GELU forms, through either entry) by (rows, width, form).  To compare the default step with a tree without the
feature, run `--kinds gelu` against both roots alternately from one shell script.  One JSON line."""
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
    ap.add_argument("--kinds", default="gelu,relu,gelu_tanh,silu")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=3, help="timed blocks per kind (the kinds take turns)")
    ap.add_argument("--profile", type=int, default=0, help="further steps per kind with every launch bracketed by timing events")
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
    modules = {"gelu": lambda: None, "relu": torch.nn.ReLU, "gelu_tanh": lambda: torch.nn.GELU(approximate="tanh"), "silu": torch.nn.SiLU}
    kinds = [k for k in args.kinds.split(",") if k]
    masker = TimeInverseBlockMasker(target_masks_per_context=4, context_mask_prob=0.65, context_mask_length=10, target_prob=0.25,
                                    target_length=10, ratio_cutoff=0.1)

    class Run:
        def __init__(self, kind):
            act = dict(activation=modules[kind]()) if kind != "gelu" else {}      # (a tree without the feature ignores the argument)
            torch.manual_seed(42)
            self.model = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=CONV_SPEC, in_channels=1),
                              transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(**act),
                              transformer_decoder_cfg=TransformerEncoderCFG.create(),
                              transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384, **act), lr=4e-4, adam_betas=(0.9, 0.98),
                              adam_weight_decay=0.04, resample_sr=16000, process_audio_seconds=2.01, nr_samples_per_audio=8,
                              average_top_k_layers=8, size="base").to(device)
            self.model.trainer.max_steps = 375000
            with pinned_mask_draws(4200):
                self.source = SyntheticAudioSource(masker, batch_size=args.clips // 8, samples_per_audio=8, n_tokens=self.model.total_patches,
                                                   seconds=10.0, seed=42, n_mask_sets=16, device=device)
            self.runner = StepRunner(self.model, gradient_clip_val=5.0)
            self.idx, self.blocks, self.out = 0, [], None

        def steps(self, n):
            torch.manual_seed(1000 + self.idx)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                self.out = self.runner.step(self.source.next_batch(), self.idx)
                self.idx += 1
            self.model._engine.wait_optimizer()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3 / n

    runs = {k: Run(k) for k in kinds}
    for r in runs.values():
        r.steps(args.warmup)
    for _ in range(args.rounds):
        for r in runs.values():
            r.blocks.append(r.steps(args.steps))
    res = dict(tag=args.tag, root=os.path.basename(os.path.abspath(args.root)), clips=args.clips, kinds={})
    for k, r in runs.items():
        res["kinds"][k] = dict(ms_per_step=round(statistics.median(r.blocks), 3), ms_per_step_blocks=[round(b, 3) for b in r.blocks],
                               final_loss=float(r.out["loss"].detach()))
    if args.profile > 0:
        gelu_forms = {ops.EPI_BIAS_GELU2: "act'+act", ops.EPI_BIAS_GELU: "act"}
        for k, r in runs.items():
            ops.PROFILE = []
            r.steps(args.profile)
            per = {}
            for fn, f, e0, e1 in ops.PROFILE:
                g = f["gemm"] if fn == "wj_gemm_bf16_act" else (f if fn == "wj_gemm_bf16" else None)
                if g is None:
                    continue
                get = (lambda n: getattr(g, n)) if fn == "wj_gemm_bf16_act" else (lambda n: g[n])
                if get("epilogue") not in gelu_forms or get("N") != 4 * get("K"):
                    continue
                key = f"M={get('M')} K={get('K')} {gelu_forms[get('epilogue')]}"
                t, n = per.get(key, (0.0, 0))
                per[key] = (t + e0.elapsed_time(e1), n + 1)
            ops.PROFILE = None
            res["kinds"][k]["linear1_us_per_launch"] = {key: round(1e3 * t / n, 1) for key, (t, n) in sorted(per.items())}
            res["kinds"][k]["linear1_ms_per_step"] = round(sum(t for t, _ in per.values()) / args.profile, 3)
            res["kinds"][k]["linear1_launches_per_step"] = sum(n for _, n in per.values()) // args.profile
    torch.cuda.synchronize()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
