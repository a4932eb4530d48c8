"""Float64 reference for the device-side noise preparation of the denoiser stage (wj_noise_prepare, wavjepa_amd/audio_prep.py
DenoiserDevicePrep) and the checks the tests apply.  TEST INFRASTRUCTURE ONLY; NumPy, no GPU.

    reference(x, F, T, cut_start, place_start)   the entry's formulas (include/wavjepa_hip.h) in float64; keyword arguments build the
                                                 MUTATIONS the helper's own test must reject
    problems(y, ref)                             shape, finite, exact zeros outside [p, p + m), max |y - ref| < 2e-6 x the RMS of
                                                 the reference over [p, p + m)
    cpu_plain_path(...)                          the loader's float32 CPU path (pre_process_noise + fade_noise + placement) with
                                                 the two draws given instead of drawn

The bound: the float32 CPU path sits at most 5.9e-7 of the RMS from this reference (measured over EDGE_CASES and at the real size,
T = 320000, F = 6400); three times that, rounded up, is 2e-6 -- the rule of tests/audio_prep_reference.py.
"""
import importlib
import io
import math
import os
import sys
import tarfile
from unittest import mock

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REL_BOUND = 2e-6
TARGET_DBFS = -14.0
T_SMALL, F_SMALL = 5000, 640


def reference(x: np.ndarray, F: int, T: int, cut_start: int = 0, place_start: int = 0, *, rms_over: str = "all", ramp_points=None,
              fade_in_on_cut: bool = False, shift: int = 0) -> dict:
    """-> dict(y [T] float64, p, m, rms of y over [p, p + m)).  Mutations: rms_over="window" (RMS of the samples that survive the cut
    only), ramp_points=R (ramps of R points over R samples instead of F), fade_in_on_cut (the fade-in also on a cut clip), shift
    (the clip placed `shift` samples late)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    assert x.ndim == 1 and n >= F and T >= F
    cut = n > T
    m, s, p = (T, int(cut_start), 0) if cut else (n, 0, int(place_start))
    assert (0 <= s < n - T) if cut else (0 <= p <= T - n)
    seg = x[s:s + m]
    src = x if rms_over == "all" else seg
    rms = math.sqrt(float(np.mean(src ** 2)))
    g = 1.0 if rms == 0 else 10.0 ** ((TARGET_DBFS - 20.0 * math.log10(rms)) / 20.0)
    R = F if ramp_points is None else int(ramp_points)
    w = g * seg
    if not cut or fade_in_on_cut:
        w[:R] *= np.linspace(0.0, 1.0, R)
    w[m - R:] *= np.linspace(1.0, 0.0, R)
    y = np.zeros(T)
    y[p + shift:p + shift + m] = w
    return dict(y=y, p=p, m=m, rms=math.sqrt(float(np.mean(y[p:p + m] ** 2))))


def distance(y: np.ndarray, ref: dict) -> float:
    """max |y - ref| over the whole row in units of the reference's RMS over [p, p + m) (absolute when that RMS is 0)."""
    d = float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref["y"])))
    return d / ref["rms"] if ref["rms"] > 0 else d


def problems(y: np.ndarray, ref: dict, rel: float = REL_BOUND) -> list:
    """What is wrong with a candidate row (an empty list: it passes)."""
    y = np.asarray(y)
    if y.shape != ref["y"].shape:
        return [f"shape {y.shape} != {ref['y'].shape}"]
    bad = []
    if not np.isfinite(y).all():
        bad.append("not finite")
    p, m = ref["p"], ref["m"]
    if np.any(y[:p] != 0.0) or np.any(y[p + m:] != 0.0):
        bad.append("not exactly 0.0 outside the clip")
    d = distance(np.nan_to_num(y), ref)
    if not d < rel:
        bad.append(f"y: {d:.3e} of the RMS >= {rel:g}")
    return bad


def cpu_plain_path(x: np.ndarray, F: int, T: int, cut_start: int = 0, place_start: int = 0) -> np.ndarray:
    """The default mode's float32 path on one clip: pre_process_noise -> fade_noise -> placement (WebAudioDataModuleDenoiser.
    _augment_sample), its cut draw replaced by `cut_start` and its placement draw by `place_start`."""
    import torch
    M = importlib.import_module("wavjepa_amd.data_modules.WebAudioDataModuleDenoiser")
    sr = 5 * F
    assert int(0.2 * sr) == F
    audio = torch.zeros(T)
    noise = M.pre_process_noise(torch.from_numpy(np.asarray(x, dtype=np.float32)))
    with mock.patch.object(torch, "randint", side_effect=lambda lo, hi, size: torch.tensor([int(cut_start)])):
        noise = M.fade_noise(noise, audio, sr)
    if audio.shape[-1] > noise.shape[-1]:
        placed = torch.zeros_like(audio)
        placed[place_start:place_start + noise.shape[-1]] = noise
        noise = placed
    return noise.numpy()


def noise_clip(n: int, seed: int, loud=None, silent: bool = False) -> np.ndarray:
    """White noise, float32, amplitude 0.05; `loud` = (lo, hi): those samples at twenty times the level."""
    if silent:
        return np.zeros(n, np.float32)
    x = np.random.default_rng(seed).uniform(-0.05, 0.05, n)
    if loud is not None:
        x[loud[0]:loud[1]] *= 20.0
    return x.astype(np.float32)


def edge_cases(T: int = T_SMALL, F: int = F_SMALL) -> list:
    """(name, clip, cut_start, place_start) at out_len T and fade_len F: the lengths at which the formulas change form."""
    n3 = 3 * T
    cases = [("n=F", noise_clip(F, 1), 0, 7),
             ("n=F+1", noise_clip(F + 1, 2), 0, 0),
             ("n=2F-1 (overlapping ramps)", noise_clip(2 * F - 1, 3), 0, T - (2 * F - 1)),
             ("n=2F", noise_clip(2 * F, 4), 0, 100),
             ("n=T-1 offset 1", noise_clip(T - 1, 5), 0, 1),
             ("n=T", noise_clip(T, 6), 0, 0),
             ("n=T+1 cut 0", noise_clip(T + 1, 7), 0, 0),
             ("n=3T last legal cut", noise_clip(n3, 8), n3 - T - 1, 0),
             ("n=3T last legal cut, loud head", noise_clip(n3, 9, loud=(0, T // 2)), n3 - T - 1, 0),
             ("silent", noise_clip(2000 if T == T_SMALL else T // 3, 10, silent=True), 0, 10)]
    return cases


# ------------------------------------------------------------------------------------------------------------ temporary shards
def _shard(path, members):
    with tarfile.open(path, "w") as tf:
        for name, data in members:
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            tf.addfile(ti, io.BytesIO(data))


def _npy(a: np.ndarray) -> bytes:
    b = io.BytesIO()
    np.save(b, a)
    return b.getvalue()


def make_denoiser_shards(root, sr: int = 32000, seconds=(2.5, 1.7, 3.1, 2.2), rates=(32000, 32000, 16000, 32000)) -> dict:
    """audio.tar (FLAC, 16 bits, mono and stereo), noise.tar (.npy float32 at `sr`: clips shorter than, longer than and far longer
    than 10 s), rir.tar (.npy [3, 2, 600]) under `root` -> dict(audio / noise / rir = shard paths, pcm = {key: (pcm [n, ch], rate,
    bits)}, noises = [clips])."""
    import flac_encoder as E
    rng = np.random.default_rng(0)
    clips, pcm = [], {}
    for i, (sec, rate) in enumerate(zip(seconds, rates)):
        n, ch = int(rate * sec), 1 + i % 2
        x = np.round(6000 * np.sin(2 * np.pi * (180 + 50 * i) * np.arange(n) / rate)[:, None] + 400 * rng.standard_normal((n, ch))).astype(np.int64)
        pcm[f"clip{i}"] = (x, rate, 16)
        clips.append((f"clip{i}.flac", E.encode(x, rate, 16, blocksize=4096, stereo="mid_side" if ch == 2 else "independent",
                                                subframes=dict(kind="fixed", order=2, porder=2))))
    _shard(os.path.join(root, "audio.tar"), clips)
    decay = np.exp(-np.arange(600) / 100.0)
    _shard(os.path.join(root, "rir.tar"), [(f"r{i}.npy", _npy((rng.standard_normal((3, 2, 600)) * decay).astype(np.float32))) for i in range(3)])
    noises = [(0.3 * rng.standard_normal(int(sr * s))).astype(np.float32) for s in (3.0, 10.5, 0.25, 12.0)]
    _shard(os.path.join(root, "noise.tar"), [(f"n{i}.npy", _npy(x)) for i, x in enumerate(noises)])
    return dict(audio=os.path.join(root, "audio.tar"), noise=os.path.join(root, "noise.tar"), rir=os.path.join(root, "rir.tar"), pcm=pcm,
                noises=noises)


def denoiser_module(shards: dict, cls=None, **kw):
    from wavjepa_amd.data_modules import WebAudioDataModuleDenoiser
    if cls is None:
        class cls(WebAudioDataModuleDenoiser):
            SHUFFLE, NUM_WORKERS, PREFETCH_FACTOR = 4, 2, 1
    args = dict(batch_size=3, with_noise=True, with_rir=True, nr_samples_per_audio=2, nr_time_points=200, seed=5)
    args.update(kw)
    dm = cls(shards["audio"], shards["rir"], shards["noise"], **args)
    dm.setup("fit")
    return dm
