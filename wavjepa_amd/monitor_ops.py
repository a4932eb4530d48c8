"""Python wrapper of libwavjepa_hip_monitor.so (include/wavjepa_hip_monitor.h) in the conventions of wavjepa_amd.ops, whose namespace
re-exports it, and merge_moments, the host-side merge of the per-rank column moments of a data-parallel run."""
from __future__ import annotations

from typing import Optional

from ._abi import LIBRARIES

Ptr = object

_DEFINES = LIBRARIES["monitor"].defines
MOMENTS_ROWS = _DEFINES["WJ_MOMENTS_ROWS"]             # rows per workgroup (one partial record each) of pass 1
MOMENTS_COLS = _DEFINES["WJ_MOMENTS_COLS"]             # columns per workgroup
MOMENTS_MAX_GROUPS = _DEFINES["WJ_MOMENTS_MAX_GROUPS"]
MOMENTS_EPS = 1e-6


def masked_moments(preds: Ptr, targets: Ptr, tgt: Ptr, out: Ptr, workspace: Ptr, *, B: int, G: int, T: int, D: int, col: Ptr = None,
                   rows: Ptr = None, n_rows: int = 0, stream: Optional[int] = None) -> None:
    """out f32 [4] = (pred_var, target_var, n, 0): mean over columns of sqrt(unbiased variance + 1e-6) of the target rows of preds
    (bf16) and of targets (fp32), rows / n_rows as in masked_mse; col (optional) f64 [2][2][D]: per-column mean and M2 of both."""
    from . import ops
    ops._run("wj_masked_moments", stream, preds=ops._p(preds), targets=ops._p(targets), tgt=ops._p(tgt), rows=ops._p(rows), out=ops._p(out),
             col=ops._p(col), workspace=ops._p(workspace), B=B, G=G, T=T, D=D, n_rows=n_rows)


def merge_moments(parts) -> float:
    """stat = mean_c sqrt(var_c + 1e-6) of the union of the parts, each (n, mean[D], M2[D]): Chan's merge in fp64, in the order given.
    A part with n = 0 contributes nothing; fewer than two rows in all give variance 0."""
    import numpy as np
    n, mean, m2 = 0.0, None, None
    for nb, mb, m2b in parts:
        nb, mb, m2b = float(nb), np.asarray(mb, dtype=np.float64), np.asarray(m2b, dtype=np.float64)
        if mean is None:
            mean, m2 = np.zeros_like(mb), np.zeros_like(mb)
        if nb == 0:
            continue
        nt = n + nb
        d = mb - mean
        mean = mean + d * (nb / nt)
        m2 = m2 + m2b + d * d * (n * nb / nt)
        n = nt
    if mean is None:
        raise ValueError("merge_moments: no parts")
    var = m2 / (n - 1.0) if n >= 2 else np.zeros_like(m2)
    return float(np.sqrt(var + MOMENTS_EPS).mean())
