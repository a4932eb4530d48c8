"""Python wrapper of libwavjepa_hip_act.so (include/wavjepa_hip_act.h) in the conventions of wavjepa_amd.ops, whose namespace re-exports
it: tensors or raw device pointers in, enqueued on PyTorch's current HIP stream, a non-zero return code raises."""
from __future__ import annotations

from typing import Optional

from ._abi import ENUMS, LIBRARIES, STRUCTS

Ptr = object
# feed-forward activation kinds (wj_act)
ACT = {k[len("WJ_ACT_"):].lower(): v for k, v in LIBRARIES["act"].enums.items()}


def gemm_act(A: Ptr, B: Ptr, C: Ptr, *, act: str, M: int, N: int, K: int, lda: int, ldb: int, ldc: int, epilogue: int = ENUMS["WJ_EPI_BIAS_GELU2"],
             C2: Ptr = None, bias: Ptr = None, schedule: Optional[int] = None, persist_cus: Optional[int] = None,
             stream: Optional[int] = None) -> None:
    """linear1's forward GEMM with the activation `act` ("gelu" | "relu" | "gelu_tanh" | "silu") in the place of the erf-GELU of
    EPI_BIAS_GELU2 (C = act'(h), C2 = act(h)) / EPI_BIAS_GELU (C = act(h)): wj_gemm_bf16_act of libwavjepa_hip_act.so
    (include/wavjepa_hip_act.h).  Row-form operands; schedule / persist_cus as gemm()."""
    from . import ops
    sched = ops._GEMM_SCHEDULE if schedule is None else int(schedule)
    g = STRUCTS["wj_gemm_args"](A=ops._p(A), B=ops._p(B), C=ops._p(C), C2=ops._p(C2), bias=ops._p(bias), lda=lda, ldb=ldb, ldc=ldc, M=M, N=N, K=K,
                                epilogue=epilogue, split_k=1, alpha=1.0, schedule=0 if sched < 0 else sched + 1,
                                persist_cus=ops._PERSIST_CUS if persist_cus is None else int(persist_cus))
    ops._run("wj_gemm_bf16_act", stream, gemm=g, act=ACT[act])
