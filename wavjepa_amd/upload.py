"""Host -> device uploads of the small per-step index / mask arrays: page-locked staging, the upload stream, one packed copy."""
from __future__ import annotations

import os
from typing import List, Sequence

import numpy as np
import torch


class _PinnedStaging:
    """A small ring of page-locked host buffers for the per-step index uploads.  A copy from PAGEABLE memory is staged by the runtime
    and holds the host until everything queued on the stream before it has run (seen in the rocprofv3 trace as 0.2 ms of idle GPU
    between the crop kernel and the first front-end kernel of every step, and as a 1.7 ms longer one-stream step when the upload was
    issued behind the queued teacher forward); from page-locked memory it is just one more stream operation.  A buffer is reused only
    after the event recorded behind its last copy has completed."""
    RING = 6

    def __init__(self):
        self.slots = []            # [tensor (uint8, pinned), event or None]
        self.next = 0

    def get(self, nbytes: int):
        if len(self.slots) < self.RING:
            self.slots.append([torch.empty(max(nbytes * 3 // 2, 1 << 20), dtype=torch.uint8, pin_memory=True), None])
            return self.slots[-1]
        slot = self.slots[self.next % self.RING]
        self.next += 1
        if slot[1] is not None:
            slot[1].synchronize()
        if slot[0].numel() < nbytes:
            slot[0] = torch.empty(nbytes * 3 // 2, dtype=torch.uint8, pin_memory=True)
        return slot


_STAGING = _PinnedStaging()
_PINNED_UPLOADS = os.environ.get("WJ_PINNED_UPLOAD", "1") != "0"     # 0: pageable staging (A/B runs)
_UPLOAD_STREAM = os.environ.get("WJ_UPLOAD_STREAM", "1") != "0"       # 0: uploads on the compute stream (A/B runs)
_UPLOAD_STREAMS: dict = {}


def _upload_stream(device):
    d = torch.device(device)
    key = d.index if d.index is not None else torch.cuda.current_device()
    if key not in _UPLOAD_STREAMS:
        _UPLOAD_STREAMS[key] = torch.cuda.Stream(device=d)
    return _UPLOAD_STREAMS[key]


def pack_upload(arrays: Sequence[np.ndarray], device) -> List[torch.Tensor]:
    """One host -> device copy for a set of small index / mask arrays (uint8 / int32): packed into one byte buffer at 256-byte offsets,
    copied once (from page-locked staging memory when the target is a GPU), returned as typed views of the device buffer (every view
    keeps it alive).  A step builds ~25 such lists (mask plan, sparse-conv row lists); as separate `.to(device)` calls each was its own
    copy kernel on the stream."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 255) // 256 * 256
    total = max(total, 256)
    on_gpu = torch.device(device).type == "cuda" and _PINNED_UPLOADS
    if on_gpu:
        slot = _STAGING.get(total)
        host = slot[0].numpy()[:total]
    else:
        host = np.zeros(total, dtype=np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if on_gpu and _UPLOAD_STREAM:
        # On a stream of its own: queued on the compute stream the copy starts only when that stream gets there, and the kernel behind it
        # waits out the copy engine's latency (~70 us of idle GPU in front of every step's conv0 launches, tools/trace_gaps.py).  The host
        # runs tens of milliseconds ahead of the GPU, so on its own stream the copy is long done when the compute stream reaches the wait.
        main = torch.cuda.current_stream(device)
        up = _upload_stream(device)
        with torch.cuda.stream(up):
            dev_buf = slot[0][:total].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(up)
        main.wait_event(slot[1])
        dev_buf.record_stream(main)
    elif on_gpu:
        dev_buf = slot[0][:total].to(device, non_blocking=True)
        slot[1] = torch.cuda.Event()
        slot[1].record(torch.cuda.current_stream(device))
    else:
        dev_buf = torch.from_numpy(host).to(device, non_blocking=True)
    out = []
    for a, o in zip(arrays, offs):
        t = dev_buf[o:o + a.nbytes]
        out.append(t.view({1: torch.uint8, 4: torch.int32}[a.dtype.itemsize]).reshape(a.shape) if a.nbytes else
                   torch.zeros(a.shape, dtype={1: torch.uint8, 4: torch.int32}[a.dtype.itemsize], device=device))
    return out
