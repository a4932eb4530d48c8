"""LayerDrop (Fan et al., "Reducing Transformer Depth on Demand with Structured Dropout"; fairseq's TransformerEncoder): in a
training-mode forward every layer of a stack is skipped for the whole batch with probability p.  Host side only -- a skipped layer
issues no launch, so there is no kernel here.

The keep decision of a layer is one more site of the dropout generator (csrc/dropout_pieces.h), restated in NumPy: Philox4x32-10
keyed by the 64-bit dropout seed, counter (element group 0, 0, stream_id = SITE | layer << 8 | stack << 16, call), draw 0 of the
eight 16-bit draws; the layer is kept iff draw >= thr = round(p * 65536).  SITE = 5: the kernels use 1..4, so a layer's keep draw
never coincides with one of its element masks.  Unlike the element masks' key, the key here is the seed itself WITHOUT the
data-parallel rank: every rank skips the same layers, so no rank waits at an all-reduce for one that drew a deeper step.  The draw
is a pure function of (seed, call, stack, layer): a resumed run continues the sequence from dropout_seed and global_step alone.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

SITE_LAYER = 5
STACK = dict(enc=0, dec=1)            # dropout_ops.DROP_STACK
_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """The generator: counter words (arrays or scalars of 32-bit values) and the two key words -> the four output words (uint64
    arrays holding 32-bit values)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK32 for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3 = p1 & _MASK32, p0 & _MASK32
        c0, c2 = n0, n2
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK32, (k1 + np.uint64(_W1)) & _MASK32
    return c0, c1, c2, c3


def check_rate(p, what: str = "layerdrop") -> float:
    """The rate as a float in [0, 1); anything else is a ValueError."""
    try:
        ok = not isinstance(p, bool) and 0.0 <= float(p) < 1.0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what} must lie in [0, 1), not {p!r}")
    return float(p)


def threshold(p: float) -> int:
    """thr = round(p * 65536), at most 65535: a layer is kept iff its draw >= thr, so the rate that is drawn is thr / 65536."""
    return min(65535, int(math.floor(float(p) * 65536.0 + 0.5)))


def stream_id(stack: int, layer: int, site: int = SITE_LAYER) -> int:
    return site | layer << 8 | stack << 16


def layer_draws(seed: int, call: int, stack: int, layers: Sequence[int], site: int = SITE_LAYER) -> np.ndarray:
    """The 16-bit draws (uint32 array) of the given layers of a stack: element group 0, draw 0."""
    sid = np.array([stream_id(stack, int(i), site) for i in layers], dtype=np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10(np.zeros_like(sid), np.zeros_like(sid), sid, np.full(sid.shape, int(call) & 0xFFFFFFFF, np.uint64),
                       seed & 0xFFFFFFFF, seed >> 32)[0]
    return (w0 & np.uint64(0xFFFF)).astype(np.uint32)


def kept_layers(seed: int, call: int, stack: str, n_layers: int, p: float) -> List[int]:
    """The sorted indices of the layers of `stack` ("enc" / "dec") that run in the forward with call counter `call`.  p = 0 keeps
    every layer and does not evaluate the generator."""
    if not p or n_layers <= 0:
        return list(range(n_layers))
    d = layer_draws(seed, call, STACK[stack], range(n_layers))
    return [int(i) for i in np.nonzero(d >= threshold(p))[0]]


def check_keep(keep: Optional[Dict[str, Sequence[int]]], n_layers: Dict[str, int]) -> Optional[Dict[str, List[int]]]:
    """Validate an explicit kept set {"enc": [...], "dec": [...]} (either key may be missing: that stack draws): sorted distinct
    layer indices of the stack.  Returns it with plain int lists, or None."""
    if keep is None:
        return None
    if not isinstance(keep, dict) or not set(keep) <= set(n_layers):
        raise ValueError(f"layerdrop_keep must be None or a dict with keys out of {sorted(n_layers)}, not {keep!r}")
    out = {}
    for stack, idx in keep.items():
        try:
            ok = all(not isinstance(i, bool) and int(i) == i for i in idx)
        except TypeError:
            ok = False
        if not ok:
            raise ValueError(f"layerdrop_keep[{stack!r}] must be a list of layer indices, not {idx!r}")
        idx = [int(i) for i in idx]
        if any(i < 0 or i >= n_layers[stack] for i in idx):
            raise ValueError(f"layerdrop_keep[{stack!r}] = {idx}: the stack has layers 0..{n_layers[stack] - 1}")
        if any(b <= a for a, b in zip(idx, idx[1:])):
            raise ValueError(f"layerdrop_keep[{stack!r}] = {idx}: the indices must be sorted and distinct")
        out[stack] = idx
    return out
