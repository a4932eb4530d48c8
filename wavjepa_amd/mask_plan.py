"""The mask plan of a JEPA step: the device-side masks and the index lists built from them on the host (NumPy), one upload."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from .upload import pack_upload


@dataclass
class MaskPlan:
    """Device-side masks + the index lists of the boolean-mask gather (reference jepa.py:399,425-428)."""
    ctx_u8: torch.Tensor    # [N, T]     1 = NOT context (key masked for the student)
    tgt_u8: torch.Tensor    # [N, G, T]  1 = target position
    vis_u8: torch.Tensor    # [N*G, T]   1 = key masked for the predictor
    keep: torch.Tensor      # int32 [n_ctx] flat (b*T+t) of context rows, ascending
    inv: torch.Tensor       # int32 [N*T]  position in `keep` or -1
    n_ctx: int
    N: int = 0              # clips, target groups per clip (= target_indices.shape[1], reference jepa.py:402-405), tokens
    G: int = 0
    T: int = 0
    # ragged execution (visible tokens only).  The student's non-context rows are dropped by jepa.py:399 and the
    # predictor's non-target rows carry zero loss weight (jepa.py:356); being key-masked they influence nothing else,
    # so the student runs on the n_ctx context rows and the predictor on the n_dec visible rows, packed per sequence.
    enc_off: Optional[torch.Tensor] = None    # int32 [N+1]     context rows before clip b
    dec_rows: Optional[torch.Tensor] = None   # int32 [n_dec]   dense (b*G+g)*T+t of every visible predictor row, ascending
    dec_off: Optional[torch.Tensor] = None    # int32 [N*G+1]
    dec_map: Optional[torch.Tensor] = None    # int32 [N*G*T]   packed row of a dense position or -1
    n_dec: int = 0
    # predictor rows whose OUTPUT is used (targets): after the last layer's attention only these go on (context rows of the
    # last layer serve as keys / values only)
    tgt_rows: Optional[torch.Tensor] = None   # int32 [n_tgt]  packed predictor row of every target, ascending
    tgt_inv: Optional[torch.Tensor] = None    # int32 [n_dec]  position in tgt_rows or -1
    tgt_dense: Optional[torch.Tensor] = None  # int32 [n_tgt]  dense (b*G+g)*T+t of those rows (loss row list)
    n_tgt: int = 0
    max_enc: int = 0                          # longest context / visible sequence (attention length bound)
    max_dec: int = 0
    ragged_ok: bool = False                   # False when a target position is key-masked: the dense path must be used
    ctx_np: Optional[np.ndarray] = None       # host copy of the context mask (True = NOT context), for the conv row lists


def make_mask_plan(ctx_mask, target_indices, vis_mask, device) -> MaskPlan:
    """Build the plan.  CPU masks (the data-loader case) need no device synchronisation."""
    if isinstance(ctx_mask, torch.Tensor) and ctx_mask.is_cuda:
        # device masks: the index lists need their sizes on the host, like the reference's x[~mask] (one sync)
        ctx_mask, target_indices, vis_mask = ctx_mask.cpu(), target_indices.cpu(), vis_mask.cpu()
    ctx_np = np.ascontiguousarray(np.asarray(ctx_mask, dtype=bool))
    tgt_np = np.ascontiguousarray(np.asarray(target_indices, dtype=bool))
    vis_np = np.ascontiguousarray(np.asarray(vis_mask, dtype=bool))
    if ctx_np.ndim != 2 or tgt_np.ndim != 3 or tgt_np.shape[0] != ctx_np.shape[0] or tgt_np.shape[2] != ctx_np.shape[1]:
        raise ValueError(f"masks: expected ctx [N, T] and target_indices [N, G, T], got {ctx_np.shape} and {tgt_np.shape}")
    n_clips, n_groups, n_tok = tgt_np.shape
    if vis_np.size != tgt_np.size or vis_np.shape[-1] != n_tok:
        raise ValueError(f"masks: ctx_and_target_masks must hold N*G*T = {tgt_np.size} entries with T last, got {vis_np.shape}")
    vis_np = vis_np.reshape(-1, n_tok)
    keep_np = np.flatnonzero(~ctx_np.reshape(-1)).astype(np.int32)
    inv_np = np.full(ctx_np.size, -1, dtype=np.int32)
    inv_np[keep_np] = np.arange(keep_np.size, dtype=np.int32)
    # ragged index lists
    ctx_len = (~ctx_np).sum(axis=-1)
    enc_off = np.concatenate([[0], np.cumsum(ctx_len)]).astype(np.int32)
    seen = ~vis_np                                             # [N*G, T] rows the predictor computes
    dec_rows = np.flatnonzero(seen.reshape(-1)).astype(np.int32)
    dec_len = seen.sum(axis=-1)
    dec_off = np.concatenate([[0], np.cumsum(dec_len)]).astype(np.int32)
    dec_map = np.full(seen.size, -1, dtype=np.int32)
    dec_map[dec_rows] = np.arange(dec_rows.size, dtype=np.int32)
    ragged_ok = (tgt_np.reshape(vis_np.shape).shape == vis_np.shape
                 and not bool(np.any(tgt_np.reshape(vis_np.shape) & vis_np)))   # every target row is also a key
    if ragged_ok:
        is_tgt = tgt_np.reshape(-1)[dec_rows]                 # per packed predictor row
        tgt_rows = np.flatnonzero(is_tgt).astype(np.int32)
        tgt_inv = np.full(dec_rows.size, -1, dtype=np.int32)
        tgt_inv[tgt_rows] = np.arange(tgt_rows.size, dtype=np.int32)
        tgt_dense = dec_rows[tgt_rows]
    else:
        tgt_rows = tgt_inv = tgt_dense = np.zeros(0, np.int32)

    d = pack_upload([ctx_np.astype(np.uint8), tgt_np.astype(np.uint8), vis_np.astype(np.uint8), keep_np.astype(np.int32),
                     inv_np.astype(np.int32), enc_off.astype(np.int32), dec_rows.astype(np.int32), dec_off.astype(np.int32),
                     dec_map.astype(np.int32), tgt_rows.astype(np.int32), tgt_inv.astype(np.int32), tgt_dense.astype(np.int32)], device)
    return MaskPlan(d[0], d[1], d[2], d[3], d[4],
                    int(keep_np.size), N=n_clips, G=n_groups, T=n_tok, enc_off=d[5], dec_rows=d[6],
                    dec_off=d[7], dec_map=d[8], n_dec=int(dec_rows.size),
                    tgt_rows=d[9], tgt_inv=d[10], tgt_dense=d[11],
                    n_tgt=int(tgt_rows.size),
                    max_enc=int(ctx_len.max()) if ctx_len.size else 0, max_dec=int(dec_len.max()) if dec_len.size else 0,
                    ragged_ok=ragged_ok, ctx_np=ctx_np)
