"""Audio preparation on the device: what the loader workers of the reference do per file after decoding
(data_modules/WebAudioDataModule.py:43-60 kaiser-sinc resampling to `sr`, dataset_functions.py:90-111 RMS -14 dBFS and the 10 s
pad / cut) as ONE HIP entry, `wj_audio_prepare` (csrc/audio_prep.hip), on a ragged batch of raw integer PCM.

    RawAudioBatch      what a worker ships in raw mode: channel-0 PCM of every clip in one flat integer buffer + rate / bit depth,
                       and the three mask tensors unchanged
    DevicePrep         raw batch -> (audio [B, 1, seconds * sr] float32 on the device, ctx, tgt, vis): the tuple
                       JEPA.on_after_batch_transfer takes.  Upload and kernels run on the engine's upload stream, into one of two
                       output buffers, so batch k + 1 is prepared while step k runs; the consumer waits on an event
    DevicePrepLoader   the iterable train_dataloader() returns in raw mode: wraps the DataLoader, prepares one batch ahead
    prepare_waveforms  the same kernel for clips held in memory

GPU only, no fallback: on a host without a HIP device every entry raises."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .resample import KAISER_BEST, sinc_resample_kernel

MAX_PHASES, MAX_TAPS = 1024, 4096         # limits of wj_audio_prepare (include/wavjepa_hip.h)
PCM, PREPARED, FLOAT_RAW = 0, 1, 2        # states of a clip in RawAudioBatch.prepared


def rate_pair(rate: int, sr: int) -> Tuple[int, int, int, int]:
    """-> (orig, new, width, taps) of the kaiser-best table for file rate `rate` and target `sr` (torchaudio's formulas)."""
    g = math.gcd(int(rate), int(sr))
    orig, new = int(rate) // g, int(sr) // g
    width = math.ceil(KAISER_BEST["lowpass_filter_width"] * orig / (min(orig, new) * KAISER_BEST["rolloff"]))
    return orig, new, width, 2 * width + orig


def device_supports(rate: int, sr: int) -> bool:
    """Whether wj_audio_prepare takes this rate pair (a loader worker prepares the other clips itself)."""
    if rate == sr:
        return True
    _, new, _, taps = rate_pair(rate, sr)
    return rate > 0 and new <= MAX_PHASES and taps <= MAX_TAPS


class RawAudioBatch:
    """A batch as a raw-mode worker ships it.  Clip b is `lengths[b]` samples at `rates[b]` Hz starting at `offsets[b]` of `pcm`
    (int16 when every PCM clip of the batch has <= 16 bits, else int32; `bits[b]` = its bit depth) -- or, with `prepared[b]` != 0, of
    the float32 buffer `f32`: PREPARED = already at the target rate, normalised and padded by the worker (the device copies it),
    FLOAT_RAW = float samples at the file rate (prepare_waveforms)."""

    def __init__(self, pcm: torch.Tensor, f32: torch.Tensor, offsets: torch.Tensor, lengths: torch.Tensor, rates: torch.Tensor,
                 bits: torch.Tensor, prepared: torch.Tensor, ctx=None, tgt=None, vis=None):
        self.pcm, self.f32, self.offsets, self.lengths, self.rates, self.bits, self.prepared = pcm, f32, offsets, lengths, rates, bits, prepared
        self.ctx, self.tgt, self.vis = ctx, tgt, vis

    def __len__(self) -> int:
        return int(self.offsets.numel())

    def clip(self, b: int) -> torch.Tensor:
        """The samples of clip b (a view)."""
        buf = self.f32 if int(self.prepared[b]) else self.pcm
        o = int(self.offsets[b])
        return buf[o:o + int(self.lengths[b])]

    def pin_memory(self) -> "RawAudioBatch":
        """For the DataLoader's pinning thread: the two sample buffers are what is uploaded."""
        self.pcm, self.f32 = self.pcm.pin_memory(), self.f32.pin_memory()
        return self

    @staticmethod
    def collate(items: Sequence[tuple]) -> "RawAudioBatch":
        """items: (samples 1-D numpy int / float32, rate, bits, state, ctx, tgt, vis) per clip."""
        wide = any(it[3] == PCM and it[2] > 16 for it in items)
        dtype = np.int32 if wide else np.int16
        offsets, lengths, n_pcm, n_f32 = [], [], 0, 0
        for it in items:
            n = int(it[0].shape[0])
            lengths.append(n)
            if it[3] == PCM:
                offsets.append(n_pcm)
                n_pcm += n
            else:
                offsets.append(n_f32)
                n_f32 += n
        pcm, f32 = np.empty(max(n_pcm, 1), dtype=dtype), np.empty(max(n_f32, 1), dtype=np.float32)
        pcm[n_pcm:], f32[n_f32:] = 0, 0
        for it, o, n in zip(items, offsets, lengths):
            (pcm if it[3] == PCM else f32)[o:o + n] = it[0]
        masks = [None if items[0][k] is None else torch.stack([it[k] for it in items]) for k in (4, 5, 6)]
        return RawAudioBatch(torch.from_numpy(pcm), torch.from_numpy(f32), torch.tensor(offsets, dtype=torch.int64),
                             torch.tensor(lengths, dtype=torch.int32), torch.tensor([it[1] for it in items], dtype=torch.int32),
                             torch.tensor([it[2] for it in items], dtype=torch.int32),
                             torch.tensor([it[3] for it in items], dtype=torch.uint8), *masks)


class _Pending:
    """A batch whose preparation is enqueued on the side stream."""

    def __init__(self, batch: tuple, done: "torch.cuda.Event"):
        self._batch, self._done = batch, done

    def get(self) -> tuple:
        """Orders the current stream behind the preparation (an event wait on the device, no host synchronise) and hands the batch out."""
        torch.cuda.current_stream(self._batch[0].device).wait_event(self._done)
        return self._batch


class DevicePrep:
    def __init__(self, sr: int = 16000, seconds: int = 10, device=None):
        self.sr, self.out_len = int(sr), int(sr) * int(seconds)
        self.device = None if device is None else torch.device(device)
        self._tables: Dict[int, tuple] = {}
        self._out: List[Optional[torch.Tensor]] = [None, None]
        self._dev: Dict[str, torch.Tensor] = {}          # device staging (pcm / f32 / workspace), used in side-stream order only
        self._host: Dict[str, list] = {}                 # page-locked staging for batches that arrive pageable: [buffer, event of its last upload]
        self._k = 0

    # ---------------------------------------------------------------------------------------------------------------- pieces
    def _device(self) -> torch.device:
        ops.require_gpu()
        if self.device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _table(self, rate: int):
        """(table on the device or None, orig, new, width, taps) of file rate `rate`, cached per instance (= per device)."""
        if rate not in self._tables:
            if rate == self.sr:
                self._tables[rate] = (None, 1, 1, 0, 1)
            else:
                kern, width, orig, new = sinc_resample_kernel(rate, self.sr, resampling_method="sinc_interp_kaiser", dtype=torch.float32,
                                                              **KAISER_BEST)
                self._tables[rate] = (torch.from_numpy(kern).to(self.device), orig, new, width, int(kern.shape[1]))
        return self._tables[rate]

    def _grown(self, key: str, n: int, dtype) -> torch.Tensor:
        t = self._dev.get(key)
        if t is None or t.dtype != dtype or t.numel() < n:
            t = self._dev[key] = torch.empty(max(n * 5 // 4, 1024), dtype=dtype, device=self.device)
        return t

    def _upload(self, key: str, host: torch.Tensor, side) -> torch.Tensor:
        """host buffer -> device staging on the side stream; pageable input goes through page-locked staging this object owns."""
        if not host.is_pinned():
            slot = self._host.get(key)
            if slot is None or slot[0].dtype != host.dtype or slot[0].numel() < host.numel():
                slot = self._host[key] = [torch.empty(max(host.numel() * 5 // 4, 1024), dtype=host.dtype, pin_memory=True), None]
            if slot[1] is not None:
                slot[1].synchronize()                  # the previous upload from this buffer has left it (long done: two batches ago)
            slot[0][:host.numel()].copy_(host)
            src = slot[0][:host.numel()]
        else:
            slot, src = None, host
        dev = self._grown(key, host.numel(), host.dtype)
        dev[:host.numel()].copy_(src, non_blocking=True)
        if slot is not None:
            slot[1] = torch.cuda.Event()
            slot[1].record(side)
        return dev

    # ---------------------------------------------------------------------------------------------------------------- API
    def prepare_async(self, raw: RawAudioBatch, normalize: bool = True) -> _Pending:
        dev = self._device()
        from .engine import _upload_stream
        side = _upload_stream(dev)
        B = len(raw)
        state, rates = raw.prepared.numpy(), raw.rates.numpy()
        offsets, lengths, bits = raw.offsets.numpy(), raw.lengths.numpy(), raw.bits.numpy()
        # the slot about to be overwritten was last read by the step two batches ago, enqueued on the compute stream before this call
        free = torch.cuda.Event()
        free.record(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            side.wait_event(free)
            slot = self._k % 2
            self._k += 1
            out = self._out[slot]
            if out is None or out.shape[0] != B:
                out = self._out[slot] = torch.empty(B, 1, self.out_len, dtype=torch.float32, device=dev)
            groups: Dict[tuple, list] = {}
            for b in range(B):
                groups.setdefault((int(state[b]), int(rates[b])), []).append(b)
            bufs = {}
            for (st, rate), clips in sorted(groups.items()):
                src = raw.pcm if st == PCM else raw.f32
                key = "pcm" if st == PCM else "f32"
                if key not in bufs:
                    bufs[key] = self._upload(key, src, side)
                if st == PREPARED and rate != self.sr:
                    raise ValueError(f"a prepared clip must be at the target rate {self.sr}, not {rate}")
                table, orig, new, width, taps = self._table(rate)
                kind = 2 if st != PCM else (0 if src.dtype == torch.int16 else 1)
                max_len = int(max(lengths[b] for b in clips))
                dims = dict(B=B, n_clips=len(clips), pcm_kind=kind, max_len=max_len, orig=orig, nw=new, width=width, taps=taps,
                            out_len=self.out_len, table=1 if table is not None else 0)
                need = ops.workspace_bytes("wj_audio_prepare", **dims)
                ws = self._grown("ws", (need + 3) // 4, torch.float32)
                dims.pop("table"), dims.pop("n_clips")
                ops.audio_prepare(bufs[key], table, out, ws, offsets=offsets, lengths=lengths, bits=None if kind == 2 else bits,
                                  clips=np.asarray(clips, dtype=np.int32), pcm_elems=int(src.numel()), workspace_bytes=ws.numel() * 4,
                                  skip_normalize=(st == PREPARED) or not normalize, stream=side.cuda_stream, **dims)
            done = torch.cuda.Event()
            done.record(side)
        return _Pending((out, raw.ctx, raw.tgt, raw.vis), done)

    def prepare(self, raw: RawAudioBatch):
        """-> (audio [B, 1, sr * seconds] float32 on the device, ctx, tgt, vis).  The audio tensor is one of two buffers this object
        owns: it is overwritten by the second prepare() after this one."""
        return self.prepare_async(raw).get()


class DevicePrepLoader:
    """Iterable over prepared batches: pulls RawAudioBatch objects from `loader` and keeps ONE batch ahead of the consumer, so the
    preparation of batch k + 1 is on the side stream before step k is enqueued."""

    def __init__(self, loader: Iterable, prep: DevicePrep):
        self.loader, self.prep = loader, prep

    def __iter__(self):
        it = iter(self.loader)
        try:
            ahead = self.prep.prepare_async(next(it))
        except StopIteration:
            return
        for raw in it:
            cur, ahead = ahead, self.prep.prepare_async(raw)
            yield cur.get()
        yield ahead.get()


_PREPS: Dict[tuple, DevicePrep] = {}


def prepare_waveforms(clips: Sequence[tuple], sr: int = 16000, seconds: int = 10, device=None, normalize: bool = True) -> torch.Tensor:
    """clips: (samples, rate) or (samples, rate, bits) per clip; samples a 1-D int16 / int32 tensor of PCM (bits defaults to the
    dtype's width) or a 1-D float32 tensor in [-1, 1).  -> [B, 1, sr * seconds] float32 on the device: each clip resampled to `sr`,
    scaled to -14 dBFS RMS (normalize=False: not scaled), zero-padded or cut -- `pre_process` of the loader, on the GPU."""
    ops.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    items = []
    for c in clips:
        x, rate = c[0], int(c[1])
        x = torch.as_tensor(x)
        if x.ndim != 1:
            raise ValueError("prepare_waveforms takes 1-D clips (one channel)")
        if x.dtype == torch.float32:
            items.append((x.numpy(), rate, 32, FLOAT_RAW, None, None, None))
        elif x.dtype in (torch.int16, torch.int32):
            bits = int(c[2]) if len(c) > 2 else (16 if x.dtype == torch.int16 else 32)
            items.append((x.numpy(), rate, bits, PCM, None, None, None))
        else:
            raise TypeError(f"prepare_waveforms: int16 / int32 PCM or float32 samples, not {x.dtype}")
    key = (dev.index, int(sr), int(seconds))
    if key not in _PREPS:
        _PREPS[key] = DevicePrep(sr, seconds, dev)
    return _PREPS[key].prepare_async(RawAudioBatch.collate(items), normalize=normalize).get()[0].clone()
