"""Python wrappers of libwavjepa_hip_dropout.so (include/wavjepa_hip_dropout.h) in the conventions of wavjepa_amd.ops, whose namespace
re-exports them: tensors or raw device pointers in, enqueued on PyTorch's current HIP stream, a non-zero return code raises."""
from __future__ import annotations

from typing import Optional

from ._abi import LIBRARIES, STRUCTS

Ptr = object


def _p(x) -> int:
    from . import ops
    return ops._p(x)


def _run(fn: str, stream: Optional[int], **fields) -> None:
    from . import ops
    ops._run(fn, stream, **fields)


DROP_SITE_ATTN, DROP_SITE_RES1, DROP_SITE_FFN, DROP_SITE_RES2 = 1, 2, 3, 4
DROP_STACK = dict(enc=0, dec=1)


def drop_args(seed: int, call: int, p: float, *, site: int, layer: int = 0, stack: int = 0):
    """The shared tail wj_dropout_args of the _drop entries: stream_id = site | layer << 8 | stack << 16."""
    return LIBRARIES["dropout"].struct_types["wj_dropout_args"](seed=int(seed) & 0xFFFFFFFFFFFFFFFF, call=int(call) & 0xFFFFFFFF,
                                                                   stream_id=(site | layer << 8 | stack << 16) & 0xFFFFFFFF, p=float(p))


def dropout_rows(x: Ptr, x2: Ptr = None, *, M: int, N: int, drop, ldx: Optional[int] = None, stream: Optional[int] = None) -> None:
    """In place: x (and x2, same mask) <- bf16(x * scale) where kept, +0 where dropped; bf16 [M][N], N % 8 == 0."""
    _run("wj_dropout_rows", stream, x=_p(x), x2=_p(x2), ldx=N if ldx is None else ldx, M=M, N=N, drop=drop)


def layernorm_fwd_drop(x: Ptr, gamma: Ptr, beta: Ptr, *, M: int, D: int, eps: float, r: Ptr, drop, y_f32: Ptr = None, y_bf16: Ptr = None,
                       mean: Ptr = None, rstd: Ptr = None, x_is_bf16: bool = False, group_stats: Ptr = None, group_rows: int = 0,
                       stream: Optional[int] = None) -> None:
    """layernorm_fwd over s = x + dropout(r)."""
    ln = STRUCTS["wj_ln_fwd_args"](x=_p(x), r=_p(r), gamma=_p(gamma), beta=_p(beta), y_f32=_p(y_f32), y_bf16=_p(y_bf16), mean=_p(mean),
                                   rstd=_p(rstd), group_stats=_p(group_stats), M=M, D=D, x_is_bf16=int(x_is_bf16), group_rows=group_rows, eps=eps)
    _run("wj_layernorm_fwd_drop", stream, ln=ln, drop=drop)


def layernorm_bwd_drop(dy: Ptr, x: Ptr, gamma: Ptr, mean: Ptr, rstd: Ptr, *, M: int, D: int, r: Ptr, drop, dy2: Ptr = None,
                       ds_f32: Ptr = None, ds_bf16: Ptr = None, dgamma: Ptr = None, dbeta: Ptr = None, dbias: Ptr = None,
                       x_is_bf16: bool = False, workspace: Ptr = None, dy2_is_bf16: bool = False, stream: Optional[int] = None) -> None:
    """layernorm_bwd of the above: ds_f32 the residual's gradient, ds_bf16 = bf16(ds o mask * scale), dbias its column sums."""
    ln = STRUCTS["wj_ln_bwd_args"](dy=_p(dy), dy2=_p(dy2), dy2_is_bf16=int(dy2_is_bf16), x=_p(x), r=_p(r), gamma=_p(gamma), mean=_p(mean),
                                   rstd=_p(rstd), ds_f32=_p(ds_f32), ds_bf16=_p(ds_bf16), dgamma=_p(dgamma), dbeta=_p(dbeta), dbias=_p(dbias),
                                   workspace=_p(workspace), M=M, D=D, x_is_bf16=int(x_is_bf16))
    _run("wj_layernorm_bwd_drop", stream, ln=ln, drop=drop)


def attn_stream_fwd_drop(qkv: Ptr, out: Ptr, *, B: int, T: int, H: int, hd: int, drop, key_mask: Ptr = None, lse: Ptr = None,
                         mask_group: int = 1, seq_off: Ptr = None, stream: Optional[int] = None) -> None:
    """attn_stream_fwd with dropout on the probabilities (any T <= 1024, hd 32 / 64)."""
    attn = STRUCTS["wj_attn_fwd_args"](qkv=_p(qkv), key_mask=_p(key_mask), seq_off=_p(seq_off), out=_p(out), lse=_p(lse), B=B, T=T, H=H, hd=hd,
                                       mask_group=mask_group)
    _run("wj_attn_stream_fwd_drop", stream, attn=attn, drop=drop)


def attn_stream_bwd_drop(qkv: Ptr, out: Ptr, dout: Ptr, lse: Ptr, dqkv: Ptr, *, B: int, T: int, H: int, hd: int, drop, key_mask: Ptr = None,
                         mask_group: int = 1, dbias: Ptr = None, dbias_ws: Ptr = None, seq_off: Ptr = None, defer_fold: bool = False,
                         stream: Optional[int] = None, deterministic: bool = False) -> None:
    """attn_stream_bwd of the above; `out` is the dropped, scaled output the forward stored."""
    attn = STRUCTS["wj_attn_bwd_args"](qkv=_p(qkv), key_mask=_p(key_mask), seq_off=_p(seq_off), out=_p(out), dout=_p(dout), lse=_p(lse),
                                       dqkv=_p(dqkv), dbias=_p(dbias), dbias_ws=_p(dbias_ws), B=B, T=T, H=H, hd=hd, mask_group=mask_group,
                                       defer_fold=int(defer_fold), deterministic=int(deterministic))
    _run("wj_attn_stream_bwd_drop", stream, attn=attn, drop=drop)
