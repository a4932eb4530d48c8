"""The attention reference helper (tests/attention_reference.py) on the host: the kernels' arithmetic emulated in torch -- fp32 scores
and sums, exp2 domain, P normalised then rounded to bf16, dS / P rounded to bf16 in front of the second product, bf16 outputs -- in the
dense, key-masked (mask_group 1 and 3) and ragged forms, for 16-wide heads, fully masked sequences and empty sequences, at small edge
shapes (T in 1, 15, 16, 17, 31, 32, 33, 150).  The emulation must pass check() in every regime at KAPPA; every mutation must be
rejected (in the flat and planted regimes: a leaked key far below the row's maximum changes nothing and need not be rejected, so the
mutations run where fp64 says they matter -- the leak picks the masked key with the largest sum_q exp(s - lse), in the planted regime the
planted one); and with the bound loosened (KAPPA x 100, or a 2^-4 max|ref| additive term) the mutation test must fail on the stated
number of its cases."""
import math

import numpy as np
import pytest
import torch

from tests import attention_reference as ar

DEV = torch.device("cpu")


def _mask(rows, T, seed, full_row=None):
    g = np.random.default_rng(seed)
    m = g.random((rows, T)) < 0.6
    m[:, 0] = False
    if full_row is not None:
        m[full_row] = True
    return m


def _off(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


CASES = {
    "none_T1": ar.fields(3, 1, 2, 32),
    "none_T17_hd64": ar.fields(3, 17, 2, 64),
    "none_T33_hd16": ar.fields(3, 33, 3, 16),
    "mask_T15": ar.fields(3, 15, 2, 32, "mask", mask=_mask(3, 15, 1)),
    "mask_T16_hd64": ar.fields(2, 16, 2, 64, "mask", mask=_mask(2, 16, 2)),
    "mask_T31_group3": ar.fields(6, 31, 2, 32, "mask", mask=_mask(2, 31, 3), mask_group=3),
    "mask_T32_hd16": ar.fields(3, 32, 4, 16, "mask", mask=_mask(3, 32, 4)),
    "mask_T33_full_sequence": ar.fields(4, 33, 2, 64, "mask", mask=_mask(4, 33, 5, full_row=2)),
    "mask_T150_group3_full": ar.fields(5, 150, 2, 32, "mask", mask=_mask(2, 150, 6, full_row=1), mask_group=3),
    "ragged_T33": ar.fields(6, 33, 2, 32, "ragged", seq_off=_off([0, 1, 33, 15, 17, 31])),
    "ragged_T150_hd64": ar.fields(5, 150, 2, 64, "ragged", seq_off=_off([150, 143, 0, 145, 16])),
    "ragged_T17_hd16_defer": ar.fields(4, 17, 4, 16, "ragged", seq_off=_off([17, 15, 0, 1]), defer_fold=True),
    "none_T32_nolse_nodbias": ar.fields(2, 32, 2, 32, lse=False, dbias=False),
}
EXTREME = ("none_T17_hd64", "none_T33_hd16", "mask_T15", "mask_T31_group3", "mask_T33_full_sequence", "mask_T150_group3_full",
           "ragged_T33", "ragged_T150_hd64")        # cases whose odd sequences have T % 16 != 0 (the padding keys the probe needs)
MUTATION_REGIMES = ("flat", "planted")


def emulate_fwd(o, write_lse=True):
    f, ix = o.f, o.ix
    H, hd, D = f["H"], f["hd"], o.D
    scale = np.float32(1.0 / math.sqrt(hd))
    scale2 = np.float32(scale * np.float32(ar.LOG2E))
    out, lse = o.view("out"), o.lse_rows().clone()
    for b in range(f["B"]):
        L, r0 = int(ix.len[b]), int(ix.row0[b])
        if L == 0:
            continue
        x = o.view("qkv")[r0:r0 + L].float().reshape(L, 3, H, hd)
        kv = ix.kval[b, :L]
        for h in range(H):
            q, k, v = x[:, 0, h], x[:, 1, h], x[:, 2, h]
            s = q @ k.t() + torch.where(kv, 0.0, float("-inf"))[None, :]
            mx = s.amax(1, keepdim=True)
            ms = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
            p = torch.exp2(s * scale2 - ms * scale2)
            sm = p.sum(1, keepdim=True)
            inv = torch.where(sm > 0, 1.0 / sm, torch.zeros_like(sm))
            P = (p * inv).to(torch.bfloat16).float()
            out[r0:r0 + L, h * hd:(h + 1) * hd] = (P @ v).to(torch.bfloat16)
            lse[r0:r0 + L, h] = torch.where(sm > 0, ms * scale + torch.log(sm), torch.full_like(sm, float("inf")))[:, 0]
    if f["lse"] and write_lse:
        o.set_lse_rows(lse, o.b["lse"].t)
    return lse


def emulate_bwd(o, lse, defer_fold=None):
    """lse [R][H]: the forward's (kept by the caller when the call itself does not ask for it)"""
    f, ix = o.f, o.ix
    H, hd, D = f["H"], f["hd"], o.D
    scale = np.float32(1.0 / math.sqrt(hd))
    dqkv, ws = o.view("dqkv"), o.view("dbias_ws")
    for b in range(f["B"]):
        L, r0 = int(ix.len[b]), int(ix.row0[b])
        if f["dbias"]:
            ws[b] = 0.0
        if L == 0:
            continue
        x = o.view("qkv")[r0:r0 + L].float().reshape(L, 3, H, hd)
        kv = ix.kval[b, :L]
        for h in range(H):
            c = slice(h * hd, (h + 1) * hd)
            q, k, v = x[:, 0, h], x[:, 1, h], x[:, 2, h]
            dO, O = o.view("dout")[r0:r0 + L, c].float(), o.view("out")[r0:r0 + L, c].float()
            p = torch.where(kv[None, :], torch.exp((q @ k.t()) * scale - lse[r0:r0 + L, h][:, None]), torch.zeros(()))
            delta = (dO * O).sum(1, keepdim=True)
            ds = (p * (dO @ v.t() - delta) * scale).to(torch.bfloat16).float()
            for j, val in enumerate((ds @ k, ds.t() @ q, p.to(torch.bfloat16).float().t() @ dO)):
                val = val.to(torch.bfloat16)
                dqkv[r0:r0 + L, j * D + h * hd:j * D + (h + 1) * hd] = val
                if f["dbias"]:
                    ws[b, j * D + h * hd:j * D + (h + 1) * hd] = val.float().sum(0)
    if f["dbias"] and not (f["defer_fold"] if defer_fold is None else defer_fold):
        o.view("dbias").add_(ws.sum(0))


def run_case(f, regime, seed=0):
    """emulated forward and backward on fresh operands: (operands, forward reference, backward reference, snapshots, outputs)"""
    o = ar.Operands(f, DEV, seed=seed, regime=regime)
    snap_f, snap_b = o.snapshot("fwd"), o.snapshot("bwd")
    lse = emulate_fwd(o)
    ex_f = ar.reference_fwd(o)
    lse_t = None
    if not f["lse"]:                                         # the backward's lse then lives in a buffer of the test's own
        lse_t = o.b["lse"].t.clone()
        o.set_lse_rows(lse, lse_t)
    emulate_bwd(o, lse)
    ex_b = ar.reference_bwd(o, ex_f, lse_t=lse_t)
    return o, ex_f, ex_b, snap_f, snap_b


PAIRS = [(n, r) for n in CASES for r in ar.REGIMES if r != "extreme" or n in EXTREME]


@pytest.mark.parametrize("name,regime", PAIRS, ids=[f"{n}-{r}" for n, r in PAIRS])
def test_emulation_is_within_the_bound(name, regime):
    o, ex_f, ex_b, snap_f, snap_b = run_case(CASES[name], regime)
    bad_f, w_f = ar.check(o, ex_f, snap_f, "fwd")
    per = dict(ar.LAST)
    bad_b, w_b = ar.check(o, ex_b, snap_b, "bwd")
    per.update(ar.LAST)
    print(f"{name} {regime}: worst err/bound " + " ".join(f"{k}={v:.3f}" for k, v in per.items())
          + (f" extreme magnitude {o.extreme_scale}" if regime == "extreme" else ""))
    assert not bad_f and not bad_b, "\n".join(bad_f + bad_b)
    # KAPPA's evidence: at KAPPA = 1 the emulation may leave the bound (the issue's trial measured up to 1.39), at KAPPA it holds
    # with a factor to spare
    assert max(w_f, w_b) < 0.5, (w_f, w_b)


def _unrejected(f, regime, **loose):
    o, ex_f, ex_b, snap_f, snap_b = run_case(f, regime)
    outs_f = {n: o.b[n].t.clone() for n in snap_f}
    outs_b = {n: o.b[n].t.clone() for n in snap_b}
    names, missed = [], []
    for what, phase, mutated in ar.mutations(o, outs_f, outs_b):
        names.append(what)
        bad, _ = ar.check(o, ex_f if phase == "fwd" else ex_b, snap_f if phase == "fwd" else snap_b, phase, mutated, **loose)
        if not bad:
            missed.append(what)
    return names, missed


MUTATED = [n for n in CASES if n != "none_T1"]              # (one key: nothing to drop or swap)


@pytest.mark.parametrize("regime", MUTATION_REGIMES)
@pytest.mark.parametrize("name", MUTATED)
def test_every_mutation_is_rejected(name, regime):
    f = CASES[name]
    names, missed = _unrejected(f, regime)
    assert not missed, f"not rejected: {missed}"
    want = {"one visible key dropped", "two V rows swapped", "last valid key dropped, first padding key admitted"}
    if f["form"] == "mask":
        want.add("one masked key let through")
    if f["hd"] == 16:
        want.add("scale of a 16-wide head taken as 1/sqrt(32)")
    have = set(names)
    for w in want:
        assert w + " (forward)" in have and w + " (backward)" in have, (w, names)
    for w in ["one 16-row query tile taken from the neighbouring head (forward)", "one sequence shifted by one row (forward)",
              "one row written one row past the region (forward)", "dq of one tile missing the scale factor (backward)",
              "a dk tile computed with dS^T (backward)", "one row written one row past the region (backward)"] + \
             (["lse of one row in log2 units (forward)"] if f["lse"] else []) + \
             (["dbias_ws row of one b added twice (backward)"] if f["dbias"] and not f["defer_fold"] else []):
        assert w in have, (w, names)


def test_a_loosened_bound_lets_mutations_through():
    """How much slack blinds the checker: of the 24 (case, regime) runs of test_every_mutation_is_rejected, the number in which at least
    one mutation passes when KAPPA is multiplied by 100, and when 2^-4 of the tensor's largest |ref| is added to every bound."""
    runs = [(n, r) for n in MUTATED for r in MUTATION_REGIMES]
    res_k = [_unrejected(CASES[n], r, kappa=ar.KAPPA * 100) for n, r in runs]
    res_n = [_unrejected(CASES[n], r, slack=2.0 ** -4) for n, r in runs]
    total = sum(len(names) for names, _ in res_k)
    got = (sum(bool(m) for _, m in res_k), sum(len(m) for _, m in res_k), sum(bool(m) for _, m in res_n), sum(len(m) for _, m in res_n))
    print(f"loosened bounds, {len(runs)} runs / {total} mutations: KAPPA x 100 misses {got[1]} mutations in {got[0]} runs, "
          f"a 2^-4 max|ref| term {got[3]} in {got[2]}")
    for (n, r), (_, mk), (_, mn) in zip(runs, res_k, res_n):
        if mk or mn:
            print(f"  {n} {r}: KAPPA x 100 misses {mk}; norm term misses {mn}")
    assert got == LOOSENED


LOOSENED = (3, 6, 2, 2)   # of 24 runs / 366 mutations: (runs, mutations) missed at KAPPA x 100, (runs, mutations) missed with the norm-wide term


def test_fully_masked_rows_have_the_documented_values():
    f = CASES["mask_T33_full_sequence"]
    o, ex_f, ex_b, snap_f, snap_b = run_case(f, "flat")
    T, D = f["T"], o.D
    rows = slice(2 * T, 3 * T)
    assert bool(ex_f.dead[rows].all()) and not bool(ex_f.dead[:2 * T].any())
    assert float(ex_f.ref["out"][rows].abs().max()) == 0.0 and float(ex_f.bound["out"][rows].abs().max()) == 0.0
    assert bool((ex_f.ref["lse"][rows] == float("inf")).all())
    assert float(ex_b.ref["dqkv"][rows].abs().max()) == 0.0 and float(ex_b.bound["dqkv"][rows].abs().max()) == 0.0
    assert float(o.view("out")[rows].float().abs().max()) == 0.0 and bool((o.lse_rows()[rows] == float("inf")).all())
    assert float(o.view("dqkv")[rows].float().abs().max()) == 0.0 and float(o.view("dbias_ws")[2].abs().max()) == 0.0
    # and the checker insists on them: a NaN, a finite lse or a nonzero gradient there is a failure
    for name, phase, val in (("out", "fwd", float("nan")), ("out", "fwd", 2.0 ** -120), ("lse", "fwd", 0.0), ("dqkv", "bwd", 2.0 ** -120)):
        t = {n: o.b[n].t.clone() for n in (snap_f if phase == "fwd" else snap_b)}
        if name == "lse":
            lr = o.lse_rows(t["lse"]).clone()
            lr[2 * T + 3, 1] = val
            o.set_lse_rows(lr, t["lse"])
        else:
            o.view(name, t[name])[2 * T + 3, 5] = val
        assert ar.check(o, ex_f if phase == "fwd" else ex_b, snap_f if phase == "fwd" else snap_b, phase, t)[0], (name, val)


def test_the_extreme_regime_reaches_the_overflow_conditions():
    """The magnitudes the overflow probe needs: every one of the hd elements of a query row and of the key rows at +-a."""
    got = {n: ar.Operands(CASES[n], DEV, regime="extreme").extreme_scale for n in ("none_T17_hd64", "mask_T15", "none_T33_hd16")}
    print("extreme magnitudes:", got)
    assert got == EXTREME_MAGNITUDES


EXTREME_MAGNITUDES = {"none_T17_hd64": 3.5, "mask_T15": 4.25, "none_T33_hd16": 5.0}     # hd 64 / 32 (key mask) / 16
