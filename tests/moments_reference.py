"""Reference, emulation, mutations and bound of the collapse monitor (wj_masked_moments, include/wavjepa_hip_monitor.h).

  reference(case, form)            fp64, from the definition: the multiset of rows (b, g, t) with target_indices[b, g, t] == 1
  emulate(case, form, mutation)    the kernel's own arithmetic on the host: the same row groups (MOMENTS_ROWS), row slots, per-thread
                                   shifted fp64 sums, slot merge (0..15, 16..31, the halves) and chain over the row groups
  MUTATIONS                        ways of getting it wrong that the bound must reject
  bounds(case, form) / violations  the yardstick is the distance of a float32 two-pass variance (x.float().var(0) on the CPU) from the
                                   fp64 reference, per column, on the same draw (bf16-rounded preds, fp32 targets); the kernel and
                                   the emulation get 4 x that distance, floored at one fp32 ulp of var + 1e-6.  The two scalars get
                                   4 x their own yardstick (torch.sqrt(x.float().var(0) + 1e-6).mean()), floored at one fp32 ulp of
                                   the statistic (out is fp32: its rounding alone is half an ulp).  A constant column must have
                                   M2 == 0 exactly, and n must be exact.
The three row forms: "dense" (preds [B*G*T][D], no row list), "ragged" (preds packed by dec_rows: every target row and the visible
context rows, which are no targets), "trimmed" (preds packed by tgt_dense: the target rows only)."""
from __future__ import annotations

import numpy as np
import torch

EPS = 1e-6
FORMS = ("dense", "ragged", "trimmed")
SLOTS = 32                      # row slots of a pass-1 workgroup (csrc/monitor.hip)
FACTOR = 4.0
# (B, G, T, D) of the kernel cases; the three around the rows-per-workgroup constant are added by kernel_cases(rows_per_workgroup)
SHAPES = [(1, 1, 1, 8), (1, 1, 2, 8), (2, 3, 37, 384), (3, 4, 50, 768), (2, 2, 33, 1000)]
# planted columns (mod D): constant, targets mean 50 / std 1e-2, preds from two bf16 neighbours, one row holding 1e3
COL_CONST, COL_OFFSET, COL_NEIGHBOURS, COL_SPIKE = 0, 1, 2, 3


def kernel_cases(rows_per_workgroup: int):
    """[(name, case)]: SHAPES with about a third of the positions targets, and three shapes whose target-row count is one less than,
    equal to and one more than rows_per_workgroup (every position a target: the trimmed list then has exactly that many rows)."""
    out = [(f"{s}", make_case(*s, seed=11 + i)) for i, s in enumerate(SHAPES)]
    for k, n in enumerate((rows_per_workgroup - 1, rows_per_workgroup, rows_per_workgroup + 1)):
        out.append((f"n={n}", make_case(1, 1, n, 16, seed=31 + k, all_targets=True)))
    return out


def make_case(B: int, G: int, T: int, D: int, seed: int, all_targets: bool = False) -> dict:
    """preds bf16 [B*G*T, D] (dense), targets f32 [B*T, D], tgt u8 [B*G*T], dec_rows / tgt_dense int32 (ascending dense indices)."""
    g = torch.Generator().manual_seed(seed)
    n_pos = B * G * T
    if all_targets:
        tgt = torch.ones(n_pos, dtype=torch.uint8)
        vis = tgt.clone()
    else:
        tgt = (torch.rand(n_pos, generator=g) < 0.35).to(torch.uint8)
        tgt[0] = 1                                          # at least one target; position 1 (if any) is decided by the draw
        if n_pos == 2:
            tgt[1] = 1
        vis = ((torch.rand(n_pos, generator=g) < 0.3).to(torch.uint8) | tgt)         # visible = targets and some context rows
    preds = (torch.randn(n_pos, D, generator=g) * 0.7 + 0.1).float()
    targets = (torch.randn(B * T, D, generator=g) * 1.3 - 0.2).float()
    # planted columns
    preds[:, COL_CONST % D] = 0.75
    targets[:, COL_CONST % D] = 3.25
    if D > COL_OFFSET:
        targets[:, COL_OFFSET] = 50.0 + 1e-2 * torch.randn(B * T, generator=g)
    if D > COL_NEIGHBOURS:
        preds[:, COL_NEIGHBOURS] = 8.0 + 2.0 ** -4 * (torch.rand(n_pos, generator=g) < 0.5).float()
    t_rows = torch.nonzero(tgt).flatten()
    if D > COL_SPIKE:
        r = int(t_rows[len(t_rows) // 2])                   # one target row holds 1e3, in preds and in its targets row
        preds[r, COL_SPIKE] = 1e3
        targets[_target_row(r, G, T), COL_SPIKE] = 1e3
    return dict(B=B, G=G, T=T, D=D, preds=preds.to(torch.bfloat16), targets=targets, tgt=tgt,
                dec_rows=torch.nonzero(vis).flatten().to(torch.int32), tgt_dense=t_rows.to(torch.int32))


def _target_row(dense: int, G: int, T: int) -> int:
    return (dense // T // G) * T + dense % T


def row_list(case: dict, form: str) -> torch.Tensor:
    """The dense index of every row of the form's preds, in order."""
    if form == "dense":
        return torch.arange(case["B"] * case["G"] * case["T"], dtype=torch.int32)
    return case["dec_rows"] if form == "ragged" else case["tgt_dense"]


def packed_preds(case: dict, form: str) -> torch.Tensor:
    """preds as the form holds them: bf16 [rows of the form][D]"""
    return case["preds"][row_list(case, form).long()].contiguous()


def gather(case: dict, form: str, mutation: str = None):
    """(P, Y) fp64 [n, D]: the multiset of target rows of preds and of targets, in the order of the form's row list."""
    G, T = case["G"], case["T"]
    rows = row_list(case, form).long()
    P = packed_preds(case, form)
    keep = torch.ones_like(rows, dtype=torch.bool) if mutation == "nontarget_rows" else case["tgt"][rows] != 0
    idx = rows[keep]
    if mutation == "bg_targets":
        y_idx = (idx // T * T + idx % T) % (case["B"] * T)       # row [b*G + g] of a [B*G][T] tensor that does not exist
    else:
        y_idx = (idx // T // G) * T + idx % T
    P, Y = P[keep].double(), case["targets"][y_idx].double()
    if mutation == "no_multiplicity":                           # a token that is a target in two groups counted once
        _, first = np.unique(y_idx.numpy(), return_index=True)
        first = torch.from_numpy(np.sort(first))
        P, Y = P[first], Y[first]
    return P, Y


def _stat(var: np.ndarray, eps: float = EPS) -> float:
    return float(np.sqrt(var + eps).mean())


def reference(case: dict, form: str) -> dict:
    """fp64: n, per-column mean / M2 / var of preds (q = 0) and targets (q = 1), and the two statistics."""
    P, Y = gather(case, form)
    n = P.shape[0]
    out = dict(n=n, mean=[], M2=[], var=[])
    for X in (P.numpy(), Y.numpy()):
        mean = X.mean(0) if n else np.zeros(case["D"])
        M2 = ((X - mean) ** 2).sum(0) if n else np.zeros(case["D"])
        out["mean"].append(mean)
        out["M2"].append(M2)
        out["var"].append(M2 / (n - 1) if n >= 2 else np.zeros(case["D"]))
    out["pred_var"], out["target_var"] = _stat(out["var"][0]), _stat(out["var"][1])
    return out


# ------------------------------------------------------------------------------------------------------------------ emulation
MUTATIONS = ("fp32_unshifted", "div_n", "no_multiplicity", "nontarget_rows", "no_eps", "bg_targets")


def _chan(n, m, M2, nb, mb, M2b):
    nt = n + nb
    f1, f2 = (nb / nt, n * nb / nt) if nt > 0 else (0.0, 0.0)
    d = mb - m
    return nt, m + d * f1, M2 + (M2b + d * d * f2)


def _thread(X: np.ndarray, mutation: str):
    """One thread's rows X [k, D] (fp64 copies of the inputs) -> (k, mean, M2): sums shifted by the first row, fp64."""
    k, D = X.shape
    if k == 0:
        return 0.0, np.zeros(D), np.zeros(D)
    if mutation == "fp32_unshifted":                             # plain fp32 sum x / sum x^2
        s1, s2 = np.zeros(D, np.float32), np.zeros(D, np.float32)
        for x in X.astype(np.float32):
            s1 = s1 + x
            s2 = s2 + x * x
        return float(k), (s1 / np.float32(k)).astype(np.float64), np.maximum(s2 - s1 * s1 / np.float32(k), 0).astype(np.float64)
    shift = X[0]
    s1, s2 = np.zeros(D), np.zeros(D)
    for x in X:
        d = x - shift
        s1 = s1 + d
        s2 = s2 + d * d
    inv = 1.0 / k
    return float(k), shift + s1 * inv, np.maximum(s2 - s1 * s1 * inv, 0.0)


def emulate(case: dict, form: str, rows_per_workgroup: int, mutation: str = None) -> dict:
    """What the two launches compute, in their order of operations: the same keys as reference()."""
    G, T, D = case["G"], case["T"], case["D"]
    rows = row_list(case, form).long()
    R = len(rows)
    on = np.ones(R, bool) if mutation == "nontarget_rows" else (case["tgt"][rows] != 0).numpy()
    y_idx = ((rows // T * T + rows % T) % (case["B"] * T)) if mutation == "bg_targets" else ((rows // T // G) * T + rows % T)
    if mutation == "no_multiplicity":
        seen, yi = set(), y_idx.numpy()
        for r in range(R):
            if on[r]:
                on[r] = yi[r] not in seen
                seen.add(yi[r])
    X = [packed_preds(case, form).double().numpy(), case["targets"][y_idx].double().numpy()]
    total = dict(n=0.0, mean=[np.zeros(D), np.zeros(D)], M2=[np.zeros(D), np.zeros(D)])
    for base in range(0, R, rows_per_workgroup):
        pos = np.arange(base, min(base + rows_per_workgroup, R))
        for q in (0, 1):
            halves = []
            for half in (0, 1):
                n, m, M2 = 0.0, np.zeros(D), np.zeros(D)
                for slot in range(half * 16, half * 16 + 16):
                    mine = pos[slot::SLOTS]
                    n, m, M2 = _chan(n, m, M2, *_thread(X[q][mine[on[mine]]], mutation))
                halves.append((n, m, M2))
            rec = _chan(*halves[0], *halves[1])
            n_all, total["mean"][q], total["M2"][q] = _chan(total["n"], total["mean"][q], total["M2"][q], *rec)
        total["n"] = n_all
    n = total["n"]
    div = n if mutation == "div_n" else n - 1
    total["var"] = [M2 / div if n >= 2 else np.zeros(D) for M2 in total["M2"]]
    eps = 0.0 if mutation == "no_eps" else EPS
    total["pred_var"], total["target_var"] = _stat(total["var"][0], eps), _stat(total["var"][1], eps)
    return total


# ---------------------------------------------------------------------------------------------------------------------- bound
def _ulp32(v):
    return np.spacing(np.asarray(v, dtype=np.float32)).astype(np.float64)


def bounds(case: dict, form: str) -> dict:
    """Yardstick distances and the bounds they give (module docstring): per column for both tensors, and for the two scalars."""
    ref = reference(case, form)
    P, Y = gather(case, form)
    out = dict(ref=ref, dist_col=[], bound_col=[], dist_stat=[], bound_stat=[])
    for q, X in enumerate((P, Y)):
        if ref["n"] >= 2:
            v32 = X.float().var(0)                              # the float32 two-pass variance (CPU)
            dist = (v32.double().numpy() - ref["var"][q]).__abs__()
            stat32 = float(torch.sqrt(v32 + EPS).mean())
        else:
            dist, stat32 = np.zeros(case["D"]), float(np.float32(np.sqrt(np.float32(EPS))))
        want = (ref["pred_var"], ref["target_var"])[q]
        out["dist_col"].append(dist)
        out["bound_col"].append(np.maximum(FACTOR * dist, _ulp32(ref["var"][q] + EPS)))
        out["dist_stat"].append(abs(stat32 - want))
        out["bound_stat"].append(max(FACTOR * abs(stat32 - want), float(_ulp32(want))))
    return out


def violations(got: dict, case: dict, form: str, bnd: dict = None) -> list:
    """What of `got` (keys of reference(); var may be absent: it is M2 / (n - 1)) lies outside the bound: [] = inside."""
    bnd = bnd or bounds(case, form)
    ref, bad = bnd["ref"], []
    n = float(got["n"])
    if n != ref["n"]:
        bad.append(f"n = {n}, reference {ref['n']}")
    const = COL_CONST % case["D"]
    for q, name in enumerate(("preds", "targets")):
        var = got["var"][q] if "var" in got else (np.asarray(got["M2"][q]) / (n - 1) if n >= 2 else np.zeros(case["D"]))
        err = np.abs(var - ref["var"][q])
        worst = int(np.argmax(err / bnd["bound_col"][q]))
        if not np.all(err <= bnd["bound_col"][q]):
            bad.append(f"{name} column {worst}: var {var[worst]!r}, reference {ref['var'][q][worst]!r}, bound {bnd['bound_col'][q][worst]:.3e}")
        if got["M2"][q][const] != 0.0:
            bad.append(f"{name} constant column {const}: M2 = {got['M2'][q][const]!r}, must be exactly 0")
        stat, want = float(got[("pred_var", "target_var")[q]]), (ref["pred_var"], ref["target_var"])[q]
        if not abs(stat - want) <= bnd["bound_stat"][q]:
            bad.append(f"{('pred_var', 'target_var')[q]} = {stat!r}, reference {want!r}, bound {bnd['bound_stat'][q]:.3e}")
    return bad
