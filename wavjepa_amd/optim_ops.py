"""Python wrapper of libwavjepa_hip_optim.so (include/wavjepa_hip_optim.h) in the conventions of wavjepa_amd.ops, whose namespace
re-exports it: tensors or raw device pointers in, enqueued on PyTorch's current HIP stream, a non-zero return code raises."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from ._abi import LIBRARIES

Ptr = object

_DEFINES = LIBRARIES["optim"].defines
ADAMW_MAX_GROUPS = _DEFINES["WJ_ADAMW_MAX_GROUPS"]       # groups of one launch
ADAMW_GRANULE = _DEFINES["WJ_ADAMW_GRANULE"]             # elements per byte of the group map (params.ALIGN)


def adamw_groups_step(p: Ptr, g: Ptr, m: Ptr, v: Ptr, n: int, *, lr: Sequence[float], weight_decay: Sequence[float], group_map: Ptr,
                      first: int, beta1: float, beta2: float, eps: float, step: int, max_norm: float = 0.0, sumsq: Ptr = None,
                      p_bf16: Ptr = None, grad_scale: float = 1.0, workgroups: int = 0, zero_grad: bool = False,
                      stream: Optional[int] = None) -> None:
    """adamw_step with lr[k] / weight_decay[k] of the group k = group_map[(first + i) // 8] of element i; p, g, m, v, p_bf16 point at
    element `first` of the flat buffers, group_map (device, uint8) at the map of the whole buffer."""
    from . import ops
    if len(lr) != len(weight_decay) or not 1 <= len(lr) <= ADAMW_MAX_GROUPS:
        raise ValueError(f"adamw_groups_step: {len(lr)} learning rates and {len(weight_decay)} weight decays; 1 .. {ADAMW_MAX_GROUPS} groups")
    table = ctypes.c_float * ADAMW_MAX_GROUPS          # (entries past n_groups stay 0: never read)
    ops._run("wj_adamw_groups_step", stream, p=ops._p(p), g=ops._p(g), m=ops._p(m), v=ops._p(v), p_bf16=ops._p(p_bf16), sumsq=ops._p(sumsq),
             n=n, beta1=beta1, beta2=beta2, eps=eps, bc1=1.0 - beta1 ** step, bc2=1.0 - beta2 ** step, max_norm=max_norm,
             grad_scale=grad_scale, workgroups=int(workgroups), zero_grad=int(zero_grad), n_groups=len(lr),
             lr=table(*[float(x) for x in lr]), weight_decay=table(*[float(x) for x in weight_decay]), group_map=ops._p(group_map),
             first=int(first))
