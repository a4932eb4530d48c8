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

Denoiser stage (wj_noise_prepare, DenoiserDevicePrep, WebAudioDataModuleDenoiser(device_prep=True)):

    prep_bench.py denoiser-worker              CPU only.  Per-sample worker cost of the denoiser data module in both modes (44.1 kHz clip)
    prep_bench.py denoiser-kernel [--reps N]   wj_noise_prepare alone (128 noise clips, half of 6 s placed, half of 14 s cut, 10 s rows
                                               at 32 kHz) and the 32 kHz wj_audio_prepare (128 x 10 s int16) alone, device-resident
                                               input, event-timed; achieved GB/s against the bytes each must move
    prep_bench.py denoiser-step [--steps N]    the denoiser step through the trainer's StepRunner, no loader: (a) ready CPU batches
                                               as the default loader delivers them, three runs; (a') raw batches + DenoiserDevicePrep
    prep_bench.py denoiser-make-shards DIR     DIR/audio (make-shards) + DIR/noise.tar (.npy, 32 kHz) + DIR/rir.tar + DIR/teacher.ckpt
                                               for `denoise.py data.device_prep=false|true` fed by 16 workers
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


def noise_batch(n_clips: int, sr: int = 32000):
    """-> (flat float32 buffer, offsets, lengths, cut_start, place_start): half the clips 6 s (placed), half 14 s (cut)."""
    rng = np.random.default_rng(0)
    T = 10 * sr
    lengths = np.array([6 * sr + 1234 if i % 2 else 14 * sr + 321 for i in range(n_clips)], np.int32)
    offsets = np.concatenate([[0], np.cumsum((lengths.astype(np.int64) + 3) // 4 * 4)[:-1]])
    flat = (0.1 * rng.standard_normal(int(offsets[-1] + lengths[-1]))).astype(np.float32)
    cut = np.array([rng.integers(0, n - T) if n > T else 0 for n in lengths], np.int32)
    place = np.array([rng.integers(0, T - n + 1) if n <= T else 0 for n in lengths], np.int32)
    return flat, offsets, lengths, cut, place


def cmd_denoiser_worker(args):
    """CPU only: per-sample worker cost of WebAudioDataModuleDenoiser in both modes, alternating, one 44.1 kHz 10 s clip."""
    import torch
    from wavjepa_amd import audio_io
    from wavjepa_amd.data_modules import WebAudioDataModuleDenoiser
    torch.set_num_threads(1)
    rng = np.random.default_rng(0)
    flac = encode(tone_clip(44100, 10.0, 1), 44100)
    noises = [torch.from_numpy((0.1 * rng.standard_normal(32000 * s)).astype(np.float32)) for s in (6, 14)]
    rirs = torch.from_numpy(rng.standard_normal((3, 2, 8000)).astype(np.float32))

    def forever(items):
        while True:
            yield from items
    dms = {m: WebAudioDataModuleDenoiser("unused", "unused", "unused", batch_size=32, with_noise=True, with_rir=True, device_prep=m) for m in (False, True)}
    rl, nl = forever([rirs]), forever(noises)
    t = {False: 0.0, True: 0.0}
    for rep in range(-1, args.reps):
        if rep == 0:
            t = {False: 0.0, True: 0.0}
        t0 = time.perf_counter()
        dms[False]._augment_sample(audio_io.decode_flac(flac), rl, nl)
        t1 = time.perf_counter()
        dms[True]._augment_raw(flac, False, rl, nl)
        t2 = time.perf_counter()
        t[False] += t1 - t0
        t[True] += t2 - t1
    off, on = (t[k] / args.reps * 1e3 for k in (False, True))
    print(f"denoiser-worker 44100 Hz: default {off:.2f} ms/sample ({1e3 / off:.1f} samples/s per worker, {16e3 / off:.0f} with 16), "
          f"raw {on:.2f} ms/sample ({1e3 / on:.1f} per worker, {16e3 / on:.0f} with 16)", flush=True)


def cmd_denoiser_kernel(args):
    import torch
    from wavjepa_amd import ops
    sr, B = 32000, 128
    T, F = 10 * sr, int(0.2 * sr)
    dev = torch.device("cuda")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    flat, offsets, lengths, cut, place = noise_batch(B, sr)
    noise, out = torch.from_numpy(flat).to(dev), torch.empty(B, T, device=dev)
    dims = dict(B=B, max_len=int(lengths.max()), out_len=T, fade_len=F)
    need = ops.workspace_bytes("wj_noise_prepare", n_clips=B, **dims)
    ws = torch.empty(need // 4, device=dev)
    ms = timed(lambda: ops.noise_prepare(noise, out, ws, offsets=offsets, lengths=lengths, cut_start=cut, place_start=place,
                                         clips=np.arange(B, dtype=np.int32), noise_elems=flat.size, workspace_bytes=need, **dims))
    m = np.minimum(lengths, T).astype(np.int64)
    moved = 4 * (int(lengths.astype(np.int64).sum()) + int(m.sum()) + B * T)
    print(f"denoiser-kernel wj_noise_prepare: {B} clips ({int(lengths.min())} / {int(lengths.max())} samples) -> {B} x {T}: {ms * 1e3:.1f} us per call "
          f"(4 launches); must move {moved / 1e6:.1f} MB (pass 1 reads every sample, pass 2 reads the kept ones and writes the rows) "
          f"-> {moved / ms / 1e6:.0f} GB/s", flush=True)

    pcm = torch.from_numpy(np.concatenate([tone_clip(sr, 10.0, i)[:, 0].astype(np.int16) for i in range(8)] * (B // 8))).to(dev)
    aoff, alen = np.arange(B, dtype=np.int64) * T, np.full(B, T, np.int32)
    adims = dict(B=B, pcm_kind=0, max_len=T, orig=1, nw=1, width=0, taps=1, out_len=T)
    aneed = ops.workspace_bytes("wj_audio_prepare", n_clips=B, table=0, **adims)
    aws, aout = torch.empty(aneed // 4, device=dev), torch.empty(B, T, device=dev)
    ms = timed(lambda: ops.audio_prepare(pcm, None, aout, aws, offsets=aoff, lengths=alen, bits=np.full(B, 16, np.int32),
                                         clips=np.arange(B, dtype=np.int32), pcm_elems=int(pcm.numel()), workspace_bytes=aneed, **adims))
    moved = B * T * (2 + 4 + 4 + 4)
    print(f"denoiser-kernel wj_audio_prepare 32 kHz (copy path): {B} x 10 s int16 -> {B} x {T}: {ms * 1e3:.1f} us per call (12 launches); must move "
          f"{moved / 1e6:.1f} MB (copy pass reads int16 and writes f32, scale pass reads and writes f32) -> {moved / ms / 1e6:.0f} GB/s", flush=True)


def _denoiser_model(batch_size: int):
    import torch
    import denoise
    from wavjepa_amd.config import load_config
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    cfg = load_config(os.path.join(ROOT, "configs"), [f"trainer.batch_size={batch_size}"], config_name="denoise")
    torch.manual_seed(0)
    tea = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=[(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)], in_channels=1),
               transformer_encoder_cfg=TransformerEncoderCFG.create(), transformer_encoder_layers_cfg=TransformerLayerCFG.create(),
               transformer_decoder_cfg=TransformerEncoderCFG.create(), transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=384),
               process_audio_seconds=2.01)
    model, _ = denoise.build_model(cfg)
    return cfg, model, tea


def cmd_denoiser_step(args):
    import torch
    from wavjepa_amd import audio_prep
    from wavjepa_amd.trainer import StepRunner
    cfg, model, tea = _denoiser_model(args.batch_size)
    model.to("cuda")
    model._set_teacher(tea.to("cuda"))
    model.train()
    runner = StepRunner(model, 1.0)
    sr, B = 32000, args.batch_size
    T = 10 * sr
    rng = np.random.default_rng(1)
    raws = []
    for k in range(2):
        flat, offsets, lengths, cut, place = noise_batch(B, sr)
        items = []
        for b in range(B):
            clean = (tone_clip(sr, 10.0, 10 * k + b)[:, 0].astype(np.int16), sr, 16, audio_prep.PCM, None, None, None)
            rirs = torch.from_numpy((rng.standard_normal((3, 2, 8000)) * np.exp(-np.arange(8000) / 1500.0)).astype(np.float32))
            items.append((clean, rirs[0], flat[offsets[b]:offsets[b] + lengths[b]], int(cut[b]), int(place[b]), rirs[1:], float(rng.uniform(-5, 5))))
        raws.append(audio_prep.RawDenoiserBatch.collate(items, T).pin_memory())
    prep = audio_prep.DenoiserDevicePrep(sr, 10, "cuda")
    ready = [tuple(t.cpu().clone() for t in prep.prepare(rb)) for rb in raws]      # what the default loader delivers (pageable CPU tensors)
    torch.cuda.synchronize()

    def feed(mode):
        if mode == "a":
            k = 0
            while True:
                yield ready[k % 2]
                k += 1
        yield from audio_prep.DevicePrepLoader((raws[i % 2] for i in range(10 ** 9)), prep)

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
    res = {"a": [], "r": []}
    for _ in range(3):
        for mode in ("a", "r"):
            res[mode].append(block(mode, args.steps))
    print(f"denoiser-step (a) ready CPU batches, no loader, {B} files per step: three runs of {args.steps} steps "
          f"{' '.join(f'{x:.2f}' for x in res['a'])} ms/step, spread {max(res['a']) - min(res['a']):.2f} ms", flush=True)
    print(f"denoiser-step (a') raw batches + DenoiserDevicePrep, no loader: {' '.join(f'{x:.2f}' for x in res['r'])} ms/step", flush=True)


def cmd_denoiser_make_shards(args):
    import torch
    cmd_make_shards(argparse.Namespace(dir=os.path.join(args.dir, "audio"), clips=args.clips))      # DIR/audio/shard-*.tar
    rng = np.random.default_rng(0)

    def put(path, arrays):
        with tarfile.open(path, "w") as tf:
            for i, a in enumerate(arrays):
                b = io.BytesIO()
                np.save(b, a)
                ti = tarfile.TarInfo(f"m{i:04d}.npy")
                ti.size = b.getbuffer().nbytes
                tf.addfile(ti, io.BytesIO(b.getvalue()))
    put(os.path.join(args.dir, "noise.tar"), [(0.1 * rng.standard_normal(32000 * s + 17 * i)).astype(np.float32) for i, s in enumerate((6, 14, 4, 12, 8, 20))])
    put(os.path.join(args.dir, "rir.tar"), [(rng.standard_normal((3, 2, 8000)) * np.exp(-np.arange(8000) / 1500.0)).astype(np.float32) for _ in range(6)])
    _, _, tea = _denoiser_model(32)
    sd = {k.replace("encoder.", "encoder._orig_mod.", 1) if k.startswith("encoder.") else k: v for k, v in tea.state_dict().items()}
    torch.save({"state_dict": sd, "hyper_parameters": {}, "global_step": 375000}, os.path.join(args.dir, "teacher.ckpt"))
    print("wrote noise.tar, rir.tar, teacher.ckpt", flush=True)


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
    p = sub.add_parser("denoiser-worker")
    p.add_argument("--reps", type=int, default=8)
    p = sub.add_parser("denoiser-kernel")
    p.add_argument("--reps", type=int, default=20)
    p = sub.add_parser("denoiser-step")
    p.add_argument("--steps", type=int, default=40)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--batch-size", type=int, default=32)
    p = sub.add_parser("denoiser-make-shards")
    p.add_argument("dir")
    p.add_argument("--clips", type=int, default=24)
    a = ap.parse_args()
    {"worker": cmd_worker, "kernel": cmd_kernel, "step": cmd_step, "make-shards": cmd_make_shards, "denoiser-worker": cmd_denoiser_worker, "denoiser-kernel": cmd_denoiser_kernel,
     "denoiser-step": cmd_denoiser_step, "denoiser-make-shards": cmd_denoiser_make_shards}[a.cmd](a)
