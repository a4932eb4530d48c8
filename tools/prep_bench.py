#!/usr/bin/env python3
"""Measurements of the device-side audio preparation (wavjepa_amd/audio_prep.py, csrc/audio_prep.hip).

    prep_bench.py worker                       CPU only.  Per-clip worker cost in both modes of WebAudioDataModule, alternating, 10 s
                                               16-bit clips at 32 and 44.1 kHz; the resampler alone; collate + pickle of a raw batch
    prep_bench.py kernel [--reps N]            32 clips of 10 s per file rate through DevicePrep.prepare; event-timed here, run it
                                               under `rocprofv3 --kernel-trace --stats -- python tools/prep_bench.py kernel` for
                                               per-kernel times.  Prints achieved fp32 FLOP/s = 2 * outputs * taps / time
    prep_bench.py step [--steps N]             step time through the trainer's StepRunner, alternating blocks: (a) ready float32
                                               batches, (b) raw 32 kHz batches + DevicePrep, (c) raw 44.1 kHz; all replayed from
                                               page-locked memory
    prep_bench.py make-shards DIR [--clips N]  44.1 kHz 10 s FLAC shards for the fed end-to-end run (train.py data.device_prep=...)
"""
import argparse
import io
import os
import pickle
import sys
import tarfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 16000
FP32_VECTOR_PEAK = 157.3e12


def tone_clip(rate: int, seconds: float, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    return np.round(6000 * np.sin(2 * np.pi * (200 + 17 * seed) * np.arange(n) / rate) + 500 * rng.standard_normal(n)).astype(np.int64)[:, None]


def encode(pcm: np.ndarray, rate: int) -> bytes:
    import flac_encoder as E
    return E.encode(pcm, rate, 16, blocksize=4096, subframes=dict(kind="fixed", order=2, porder=2))


def masker():
    from wavjepa_amd.masking import TimeInverseBlockMasker
    return TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1)


def cmd_worker(args):
    import torch
    from wavjepa_amd import audio_io, audio_prep
    from wavjepa_amd.data_modules import WebAudioDataModule
    from wavjepa_amd.resample import KAISER_BEST, resample_waveform_cpu
    torch.set_num_threads(1)
    for rate in (32000, 44100):
        flac = encode(tone_clip(rate, 10.0, 1), rate)
        dms = {m: WebAudioDataModule(masker(), "unused", None, batch_size=32, nr_samples_per_audio=8, nr_time_points=200, sr=SR, device_prep=m)
               for m in (False, True)}
        wav = audio_io.decode_flac(flac)[0][0]
        t = {False: 0.0, True: 0.0, "resample": 0.0}
        for rep in range(-1, args.reps):                 # alternating, so drift of the host hits all three alike; rep -1 warms up (imports)
            if rep == 0:
                t = {False: 0.0, True: 0.0, "resample": 0.0}
            t0 = time.perf_counter()
            dms[False]._retrieve_sample(audio_io.decode_flac(flac))
            t1 = time.perf_counter()
            item = dms[True]._retrieve_raw(flac, False)
            t2 = time.perf_counter()
            resample_waveform_cpu(wav, rate, SR, resampling_method="sinc_interp_kaiser", **KAISER_BEST)
            t3 = time.perf_counter()
            t[False] += t1 - t0
            t[True] += t2 - t1
            t["resample"] += t3 - t2
        off, on, rs = (t[k] / args.reps * 1e3 for k in (False, True, "resample"))
        t0 = time.perf_counter()
        for _ in range(10):
            batch = audio_prep.RawAudioBatch.collate([item] * 32)
        coll = (time.perf_counter() - t0) / 10 * 1e3
        t0 = time.perf_counter()
        for _ in range(10):
            pickle.loads(pickle.dumps(batch))
        pick = (time.perf_counter() - t0) / 10 * 1e3
        print(f"worker {rate} Hz: default {off:.2f} ms/clip ({1e3 / off:.1f} clips/s), raw {on:.2f} ms/clip ({1e3 / on:.1f} clips/s), "
              f"resampler alone {rs:.2f} ms; saving {off - on:.2f} ms = {(off - on) / rs:.2f} x resampler; "
              f"raw batch of 32: collate {coll:.2f} ms, pickle round trip {pick:.2f} ms ({batch.pcm.numel() * 2 / 1e6:.1f} MB int16)", flush=True)
        assert off - on >= 0.8 * rs, "raw mode must save at least 0.8 x the resample time"


def raw_batch(rate: int, n_clips: int, seconds: float, pin: bool, n_times: int = 200):
    import torch
    from wavjepa_amd import audio_prep
    m = masker()
    items = []
    for i in range(n_clips):
        ctx, tgt, vis = m(batch_size=8, n_times=n_times, in_channels=1)
        items.append((tone_clip(rate, seconds, i)[:, 0].astype(np.int16), rate, 16, audio_prep.PCM, ctx, tgt, vis))
    rb = audio_prep.RawAudioBatch.collate(items)
    return rb.pin_memory() if pin and torch.cuda.is_available() else rb


def cmd_kernel(args):
    import torch
    from wavjepa_amd import audio_prep
    prep = audio_prep.DevicePrep(SR, 10, "cuda")
    for rate in (44100, 22050, 11025, 48000, 32000, 24000, 8000, 16000):
        rb = raw_batch(rate, 32, 10.0, pin=True)
        for _ in range(3):
            prep.prepare(rb)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            prep.prepare(rb)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.reps
        taps = audio_prep.rate_pair(rate, SR)[3] if rate != SR else 0
        flop = 2.0 * 32 * 160000 * taps
        print(f"kernel {rate} Hz: prepare (upload + 3 kernels) of 32 x 10 s {ms:.3f} ms, taps {taps}, "
              f"{flop / 1e9:.2f} GFLOP -> {flop / ms / 1e9:.2f} TFLOP/s over the whole call = {100 * flop / (ms * 1e-3) / FP32_VECTOR_PEAK:.1f} % "
              f"of the fp32 vector peak", flush=True)


def cmd_step(args):
    import torch
    import train
    from wavjepa_amd import audio_prep
    from wavjepa_amd.config import load_config
    from wavjepa_amd.trainer import StepRunner
    cfg = load_config(os.path.join(ROOT, "configs"), ["trainer.batch_size=32"])
    torch.manual_seed(0)
    model, patches = train.build_model(cfg)
    model.to("cuda")
    model.train()
    runner = StepRunner(model, 5.0)
    prep = audio_prep.DevicePrep(SR, 10, "cuda")
    raws = {r: [raw_batch(r, 32, 10.0, pin=True, n_times=patches) for _ in range(2)] for r in (32000, 44100)}
    ready = []
    for rb in raws[32000]:
        a, c, t, v = prep.prepare(rb)
        ready.append((a.cpu().pin_memory(), c, t, v))
    torch.cuda.synchronize()

    def feed(mode):
        k = 0
        if mode == "a":
            while True:
                yield ready[k % 2]
                k += 1
        loader = audio_prep.DevicePrepLoader((raws[32000 if mode == "b" else 44100][i % 2] for i in range(10 ** 9)), prep)
        yield from loader

    def block(mode, n):
        it = feed(mode)
        for _ in range(3):
            runner.step(next(it), model.global_step)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            runner.step(next(it), model.global_step)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for _ in range(args.warmup):
        runner.step(ready[0], model.global_step)
    res = {"a": [], "b": [], "c": []}
    per = max(args.steps // args.blocks, 1)
    for _ in range(args.blocks):
        for mode in ("a", "b", "c"):
            res[mode].append(block(mode, per))
    for mode, name in (("a", "ready float32 batches"), ("b", "device_prep 32 kHz"), ("c", "device_prep 44.1 kHz")):
        print(f"step ({mode}) {name}: blocks of {per} steps {' '.join(f'{x:.2f}' for x in res[mode])} ms/step, mean {np.mean(res[mode]):.2f}", flush=True)
    a = np.mean(res["a"])
    print(f"step: (b) - (a) = {np.mean(res['b']) - a:+.2f} ms, (c) - (a) = {np.mean(res['c']) - a:+.2f} ms; spread of (a) against itself "
          f"{max(res['a']) - min(res['a']):.2f} ms", flush=True)


def cmd_make_shards(args):
    os.makedirs(args.dir, exist_ok=True)
    per = 8
    for s in range((args.clips + per - 1) // per):
        with tarfile.open(os.path.join(args.dir, f"shard-{s:03d}.tar"), "w") as tf:
            for i in range(s * per, min(args.clips, (s + 1) * per)):
                data = encode(tone_clip(44100, 10.0, i), 44100)
                ti = tarfile.TarInfo(f"clip{i:04d}.flac")
                ti.size = len(data)
                tf.addfile(ti, io.BytesIO(data))
        print(f"wrote shard {s}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("worker")
    p.add_argument("--reps", type=int, default=8)
    p = sub.add_parser("kernel")
    p.add_argument("--reps", type=int, default=20)
    p = sub.add_parser("step")
    p.add_argument("--steps", type=int, default=200)
    p.add_argument("--blocks", type=int, default=4)
    p.add_argument("--warmup", type=int, default=10)
    p = sub.add_parser("make-shards")
    p.add_argument("dir")
    p.add_argument("--clips", type=int, default=24)
    a = ap.parse_args()
    {"worker": cmd_worker, "kernel": cmd_kernel, "step": cmd_step, "make-shards": cmd_make_shards}[a.cmd](a)
