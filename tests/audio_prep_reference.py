"""Float64 references for the device-side audio preparation (wj_audio_prepare, wavjepa_amd/audio_prep.py) and the checks the
tests apply.  TEST INFRASTRUCTURE ONLY; NumPy, no GPU.

Two references, because the tap TABLE and the SUM are different sources of error and only the second is the kernel's:

  same_table_reference   the entry's formulas (include/wavjepa_hip.h) in float64 WITH the product's float32 table: the kernel differs
                         from it by float32 accumulation (and the float32 gain) only.  Bound: max |y - ref| < 1e-5 * rms(ref over
                         the un-padded part) -- three times the largest value of a CPU emulation of the float32 tap sum (3.4e-6 at
                         44.1 kHz), the room a different fixed grouping of the sum and the fp32 gain may take.
  oracle_reference       oracle.resample_oracle.resample (float64 table) + float64 loudness and padding.  Here the float32 table
                         dominates and no fixed number holds across rates, so the check is the yardstick form on the same input:
                         d(candidate, oracle) <= 1.1 * d(CPU product path, oracle) + 1e-5 * rms.

Both return a dict: r (resampled, padded / cut to out_len, NOT scaled -- the loudness gain cancels the PCM scale, so a wrong
2^-bits shows in r only), y (the prepared row), n_valid (= min(out_len, resampled length)), rms (of y over its un-padded part).
"""
import math
import os
import sys
from functools import lru_cache

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REL_BOUND = 1e-5
TARGET_DBFS = -14.0


@lru_cache(maxsize=None)
def product_table(rate: int, sr: int):
    import torch
    from wavjepa_amd.resample import KAISER_BEST, sinc_resample_kernel
    kern, width, orig, new = sinc_resample_kernel(rate, sr, resampling_method="sinc_interp_kaiser", dtype=torch.float32, **KAISER_BEST)
    return kern.astype(np.float64), width, orig, new


def _apply_table(x: np.ndarray, table: np.ndarray, width: int, orig: int, new: int) -> np.ndarray:
    """r[i * new + p] = sum_k table[p][k] * xpad[i * orig + k], cut to ceil(new * L / orig); float64, frames in blocks."""
    L = x.shape[0]
    target = int(math.ceil(new * L / orig))
    frames = (target + new - 1) // new
    taps = table.shape[1]
    pad = np.zeros(max((frames - 1) * orig + taps, width + L + width + orig))
    pad[width:width + L] = x
    out = np.empty((frames, new))
    view = np.lib.stride_tricks.sliding_window_view(pad, taps)[::orig]
    for lo in range(0, frames, 8192):
        out[lo:lo + 8192] = view[lo:min(frames, lo + 8192)] @ table.T
    return out.reshape(-1)[:target]


def _finish(r: np.ndarray, out_len: int, rms_over: str = "all") -> dict:
    head = r[:out_len]
    src = r if rms_over == "all" else head
    rms = math.sqrt(float(np.mean(src ** 2))) if src.size else 0.0
    gain = 1.0 if rms == 0 else 10.0 ** ((TARGET_DBFS - 20.0 * math.log10(rms)) / 20.0)
    n = head.shape[0]
    rp, y = np.zeros(out_len), np.zeros(out_len)
    rp[:n], y[:n] = head, head * gain
    return dict(r=rp, y=y, n_valid=n, rms=math.sqrt(float(np.mean(y[:n] ** 2))) if n else 0.0)


def same_table_reference(pcm: np.ndarray, bits: int, rate: int, sr: int, out_len: int, *, scale_bits=None, rms_over: str = "all",
                         swap_phase=None) -> dict:
    """pcm: 1-D integers (or float samples with bits = 0).  The keyword arguments build the MUTATIONS the helper's own test must
    reject: scale_bits (scale 2^-scale_bits), rms_over="head" (RMS of the first out_len samples only), swap_phase=p (phase p computed
    with the table row of phase p + 1)."""
    x = np.asarray(pcm, dtype=np.float64) * (1.0 if bits == 0 else 2.0 ** -((bits - 1) if scale_bits is None else scale_bits))
    if rate == sr:
        r = x
    else:
        table, width, orig, new = product_table(rate, sr)
        if swap_phase is not None:
            table = table.copy()
            table[swap_phase] = table[(swap_phase + 1) % new]
        r = _apply_table(x, table, width, orig, new)
    return _finish(r, out_len, rms_over)


def oracle_reference(pcm: np.ndarray, bits: int, rate: int, sr: int, out_len: int) -> dict:
    from oracle import resample_oracle as RS
    if not hasattr(RS.kernel, "cache_info"):
        RS.kernel = lru_cache(maxsize=None)(RS.kernel)        # its float64 table is a Python loop per tap (minutes at 640 phases): once per pair
    x = np.asarray(pcm, dtype=np.float64) * (1.0 if bits == 0 else 2.0 ** -(bits - 1))
    return _finish(RS.resample(x, rate, sr), out_len)


def cpu_product_path(pcm: np.ndarray, bits: int, rate: int, sr: int, out_len: int) -> np.ndarray:
    """The loader's default path on the same clip: decode scale -> resample_waveform_cpu -> pre_process -> [out_len] float32."""
    import torch
    from wavjepa_amd.data_modules.dataset_functions import normalize_audio, pad_or_truncate
    from wavjepa_amd.resample import KAISER_BEST, resample_waveform_cpu
    wav = torch.from_numpy(np.asarray(pcm).astype(np.float32) * np.float32(1.0 / float(1 << (bits - 1))))
    if rate != sr:
        wav = resample_waveform_cpu(wav, rate, sr, resampling_method="sinc_interp_kaiser", **KAISER_BEST)
    return pad_or_truncate(normalize_audio(wav, TARGET_DBFS).reshape(1, -1), out_len)[0].numpy()


def distance(y: np.ndarray, ref: dict, key: str = "y") -> float:
    """max |y - ref| over the whole row, in units of the RMS of the reference's un-padded part (absolute when that RMS is 0)."""
    n = ref["n_valid"]
    scale = math.sqrt(float(np.mean(ref[key][:n] ** 2))) if n else 0.0
    d = float(np.max(np.abs(np.asarray(y, dtype=np.float64) - ref[key])))
    return d / scale if scale > 0 else d


def problems(y: np.ndarray, ref: dict, r: np.ndarray = None, rel: float = REL_BOUND) -> list:
    """What is wrong with a candidate against a same-table reference (an empty list: it passes).  y: the prepared row; r: the
    un-scaled resampled row (skip_normalize), checked when given."""
    bad = []
    y = np.asarray(y)
    if y.shape != ref["y"].shape:
        return [f"shape {y.shape} != {ref['y'].shape}"]
    if not np.isfinite(y).all():
        bad.append("not finite")
    if np.any(y[ref["n_valid"]:] != 0.0):
        bad.append("padding is not exactly 0.0")
    d = distance(np.nan_to_num(y), ref)
    if not d < rel:
        bad.append(f"y: {d:.3e} of the RMS >= {rel:g}")
    if r is not None:
        dr = distance(np.nan_to_num(np.asarray(r)), ref, "r")
        if not dr < rel:
            bad.append(f"r: {dr:.3e} of the RMS >= {rel:g}")
    return bad


def level_db(y: np.ndarray, n_valid: int) -> float:
    """RMS level of the un-padded part in dBFS."""
    return 20.0 * math.log10(math.sqrt(float(np.mean(np.asarray(y[:n_valid], dtype=np.float64) ** 2))))


def noise_pcm(n: int, bits: int, seed: int, channels: int = 1, loud_tail: int = 0) -> np.ndarray:
    """White-noise PCM [n, channels] at a quarter of full scale; the last `loud_tail` samples at full scale."""
    rng = np.random.default_rng(seed)
    full = float(1 << (bits - 1)) - 1
    x = rng.uniform(-0.25, 0.25, size=(n, channels))
    if loud_tail:
        x[n - loud_tail:] = rng.uniform(-1.0, 1.0, size=(loud_tail, channels))
    return np.round(x * full).astype(np.int64)
