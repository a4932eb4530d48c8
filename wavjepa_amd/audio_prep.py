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

The denoiser stage (data_modules/WebAudioDataModuleDenoiser.py, `device_prep=True`) adds the noise branch, `wj_noise_prepare`
(csrc/noise_prep.hip: -14 dBFS over the whole noise clip, random cut or fade-in + placement, fade-out):

    RawDenoiserBatch     a RawAudioBatch of the clean clips + every noise clip as it came from its `.npy` member in one flat float32
                         buffer with the worker's draws (cut position, placement), and the RIR / SNR fields unchanged
    DenoiserDevicePrep   raw batch -> the 7-tuple Denoiser.on_after_batch_transfer takes, audio [B, T] and noise [B, T] on the device;
                         DevicePrep(32000, 10) for the clean clips, same stream, same two-buffer scheme; DevicePrepLoader takes either

GPU only, no fallback: on a host without a HIP device every entry raises."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .resample import KAISER_BEST, sinc_resample_kernel
from .upload import _upload_stream

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

    def __init__(self, batch: tuple, done: "torch.cuda.Event", fresh: Sequence[torch.Tensor] = ()):
        self._batch, self._done, self._fresh = batch, done, fresh

    def get(self) -> tuple:
        """Orders the current stream behind the preparation (an event wait on the device, no host synchronise) and hands the batch out.
        `fresh`: tensors allocated on the side stream for this batch alone; the allocator learns that the current stream reads them."""
        cur = torch.cuda.current_stream(self._batch[0].device)
        cur.wait_event(self._done)
        for t in self._fresh:
            t.record_stream(cur)
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


class RawDenoiserBatch:
    """A denoiser batch as a raw-mode worker ships it.  `clean`: the clean clips (a RawAudioBatch without masks).  Noise clip b is
    `noise_lengths[b]` float32 samples at the target rate starting at `noise_offsets[b]` of `noise` (every offset a multiple of
    four floats), exactly as its `.npy` member held them; `cut_start[b]` is the worker's draw for a clip longer than `out_len`,
    `place_start[b]` for a shorter one (0 where not drawn).  `source_rir` [B, C, L], `noise_rirs` [B, n, C, L] and `snr` [B] are
    what the default mode's collate makes of them: a field the configuration turns off is a list of None (then `noise` holds one
    zero and the lengths are 0)."""

    def __init__(self, clean: RawAudioBatch, noise: torch.Tensor, noise_offsets: torch.Tensor, noise_lengths: torch.Tensor,
                 cut_start: torch.Tensor, place_start: torch.Tensor, source_rir, noise_rirs, snr, out_len: int):
        self.clean, self.noise, self.noise_offsets, self.noise_lengths = clean, noise, noise_offsets, noise_lengths
        self.cut_start, self.place_start = cut_start, place_start
        self.source_rir, self.noise_rirs, self.snr, self.out_len = source_rir, noise_rirs, snr, int(out_len)

    def __len__(self) -> int:
        return len(self.clean)

    @property
    def has_noise(self) -> bool:
        return isinstance(self.snr, torch.Tensor)

    @property
    def noise_length(self) -> torch.Tensor:
        """m: the samples of each noise clip that land in its row (int64 [B], the default mode's `noise_length`)."""
        return self.noise_lengths.to(torch.int64).clamp(max=self.out_len)

    @property
    def noise_start_idx(self) -> torch.Tensor:
        """p (int64 [B], the default mode's `noise_start_idx`)."""
        return self.place_start.to(torch.int64)

    def noise_clip(self, b: int) -> torch.Tensor:
        o = int(self.noise_offsets[b])
        return self.noise[o:o + int(self.noise_lengths[b])]

    def pin_memory(self) -> "RawDenoiserBatch":
        """For the DataLoader's pinning thread: the sample buffers are what is uploaded in bulk."""
        self.clean, self.noise = self.clean.pin_memory(), self.noise.pin_memory()
        return self

    @staticmethod
    def collate(items: Sequence[tuple], out_len: int) -> "RawDenoiserBatch":
        """items: (clean item of RawAudioBatch.collate, source_rir | None, noise 1-D float32 numpy | None, cut_start, place_start,
        noise_rirs | None, snr | None) per sample."""
        clean = RawAudioBatch.collate([it[0] for it in items])
        offsets, lengths, total = [], [], 0
        for it in items:
            n = 0 if it[2] is None else int(it[2].shape[0])
            offsets.append(total)
            lengths.append(n)
            total += (n + 3) // 4 * 4                                   # 16-byte aligned clips: aligned dwordx4 loads in pass 1
        noise = np.zeros(max(total, 1), dtype=np.float32)
        for it, o, n in zip(items, offsets, lengths):
            if n:
                noise[o:o + n] = it[2]

        def column(k):
            col = [it[k] for it in items]
            if any(c is None for c in col):
                return col
            return torch.stack(col) if isinstance(col[0], torch.Tensor) else torch.tensor(col)
        return RawDenoiserBatch(clean, torch.from_numpy(noise), torch.tensor(offsets, dtype=torch.int64),
                                torch.tensor(lengths, dtype=torch.int32), torch.tensor([int(it[3]) for it in items], dtype=torch.int32),
                                torch.tensor([int(it[4]) for it in items], dtype=torch.int32), column(1), column(5), column(6), out_len)


class DenoiserDevicePrep:
    FADE_SECONDS = 0.2                  # generate_scenes.py:132-154

    def __init__(self, sr: int = 32000, seconds: int = 10, device=None):
        self.clean = DevicePrep(sr, seconds, device)
        self.sr, self.out_len, self.fade_len = self.clean.sr, self.clean.out_len, int(self.FADE_SECONDS * int(sr))
        self._noise: List[Optional[torch.Tensor]] = [None, None]
        self._k = 0

    def prepare_async(self, raw: RawDenoiserBatch) -> _Pending:
        if raw.out_len != self.out_len:
            raise ValueError(f"the batch was drawn for rows of {raw.out_len} samples, this object prepares {self.out_len}")
        pending = self.clean.prepare_async(raw.clean)         # (raises without a GPU); the side stream now waits for the step two batches ago
        dev = self.clean.device
        side = _upload_stream(dev)
        B = len(raw)
        audio = pending._batch[0][:, 0]
        fresh: List[torch.Tensor] = []

        def up(t):
            if not isinstance(t, torch.Tensor):
                return t
            fresh.append(t.to(dev, non_blocking=True))
            return fresh[-1]
        with torch.cuda.stream(side):
            slot = self._k % 2
            self._k += 1
            noise = [None] * B
            if raw.has_noise:
                noise = self._noise[slot]
                if noise is None or noise.shape[0] != B:
                    noise = self._noise[slot] = torch.empty(B, self.out_len, dtype=torch.float32, device=dev)
                lengths = raw.noise_lengths.numpy()
                max_len = int(lengths.max())
                src = self.clean._upload("noise", raw.noise, side)
                need = ops.workspace_bytes("wj_noise_prepare", B=B, n_clips=B, max_len=max_len, out_len=self.out_len, fade_len=self.fade_len)
                if need < 0:
                    raise ValueError(f"wj_noise_prepare refuses clips of at most {max_len} samples with a fade of {self.fade_len}")
                ws = self.clean._grown("noise_ws", (need + 3) // 4, torch.float32)
                ops.noise_prepare(src, noise, ws, offsets=raw.noise_offsets.numpy(), lengths=lengths, cut_start=raw.cut_start.numpy(),
                                  place_start=raw.place_start.numpy(), clips=np.arange(B, dtype=np.int32), noise_elems=int(raw.noise.numel()),
                                  workspace_bytes=ws.numel() * 4, B=B, max_len=max_len, out_len=self.out_len, fade_len=self.fade_len,
                                  stream=side.cuda_stream)
            batch = (audio, up(raw.source_rir), noise, up(raw.noise_length), up(raw.noise_start_idx), up(raw.noise_rirs), up(raw.snr))
            done = torch.cuda.Event()
            done.record(side)
        return _Pending(batch, done, fresh)

    def prepare(self, raw: RawDenoiserBatch):
        """-> (audio [B, T] float32 on the device, source_rir, noise [B, T], noise_length, noise_start_idx, noise_rirs, snr): the batch
        of Denoiser.on_after_batch_transfer.  audio and noise are buffers this object owns, overwritten by the second prepare() after
        this one."""
        return self.prepare_async(raw).get()


class DevicePrepLoader:
    """Iterable over prepared batches: pulls RawAudioBatch (RawDenoiserBatch) objects from `loader` and keeps ONE batch ahead of the
    consumer, so the preparation of batch k + 1 is on the side stream before step k is enqueued.  `prep`: a DevicePrep or a
    DenoiserDevicePrep."""

    def __init__(self, loader: Iterable, prep):
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
