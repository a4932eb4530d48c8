"""The GEMM reference helper (tests/gemm_reference.py) on the host: every kernel form emulated on the CPU -- fp32 accumulation over
k blocks of 32, bias added first or last, the header's rounding points, bf16 rounding by torch -- at small shapes that cross the
edges (M, N and K tails, N % 256 in {0, 8, 128, 136}, lda > K, ldc > N, overlapping row windows, rowmaps with gaps and runs,
seg_valid < seg_rows).  The emulation must pass every check; every mutation of its output, and every write outside the output region,
must be rejected."""
import math

import numpy as np
import pytest
import torch

from tests import gemm_reference as gr


def gemm_case(M, N, K, lda, ldb, ldc, epilogue="BF16", a_trans=0, b_trans=0, split_k=1, bias=False, C2=False, aux=False,
              colsum=False, rowmap=None, seg_rows=0, seg_valid=0, alpha=1.0):
    return dict(entry="gemm", unknown=(), M=M, N=N, K=K, lda=lda, ldb=ldb, ldc=ldc, epilogue=epilogue, a_trans=a_trans, b_trans=b_trans,
                split_k=split_k, bias=bias, C=True, C2=C2, aux=aux, colsum=colsum, rowmap=rowmap, seg_rows=seg_rows, seg_valid=seg_valid,
                alpha=alpha, workspace=False, schedule=None, persist_cus=None, align=(("A", 16), ("B", 2064), ("C", 4080)))


def fp8_case(M, N, K, epilogue="BF16", bias=True, C=True, C2=False, q_out=False):
    return dict(entry="gemm_mxfp8", unknown=(), M=M, N=N, K=K, lda=K, ldb=K, ldc=N, epilogue=epilogue, a_trans=0, b_trans=0, split_k=1,
                bias=bias, C=C, C2=C2, aux=False, colsum=False, rowmap=None, seg_rows=0, seg_valid=0, alpha=1.0, workspace=False,
                schedule=None, persist_cus=None, ld_scale_a=M + 3, ld_scale_b=N, q_out=q_out, ld_q_scale=M, align=())


def _rowmap_gaps_and_runs(n, first, seed):
    """sorted storage rows >= first: runs of consecutive rows separated by gaps"""
    g = np.random.default_rng(seed)
    rows, r = [], first
    while len(rows) < n:
        run = int(g.integers(1, 5))
        rows += list(range(r, r + run))
        r += run + int(g.integers(1, 4))
    return np.array(rows[:n], dtype=np.int32)


_KG = _rowmap_gaps_and_runs(40, 0, 3)
CASES = {
    "NN_bf16_bias_N8_lda_ldc": gemm_case(67, 264, 72, 80, 72, 272, bias=True),
    "NN_bias_gelu2_N128": gemm_case(40, 384, 64, 64, 64, 384, "BIAS_GELU2", bias=True, C2=True),
    "NN_bias_gelu_N0": gemm_case(33, 256, 40, 40, 40, 256, "BIAS_GELU", bias=True),
    "NN_mul_gelu_grad_colsum_N136": gemm_case(50, 392, 48, 48, 48, 400, "MUL_GELU_GRAD", aux=True, colsum=True),
    "NN_bf16_colsum_N8": gemm_case(300, 8, 40, 40, 40, 8, colsum=True),
    "NT_add_f32": gemm_case(45, 136, 56, 56, 144, 136, "ADD_F32", b_trans=1, aux=True),
    "TT_atomic_split3": gemm_case(64, 264, 150, 72, 264, 264, "ATOMIC_F32", a_trans=1, b_trans=1, split_k=3, alpha=0.5),
    "TN_bf16": gemm_case(24, 128, 40, 24, 40, 128, a_trans=1),
    "NN_conv_gelu_overlapping": gemm_case(33, 32, 96, 64, 96, 40, "CONV_GELU", C2=True, seg_rows=11, seg_valid=9),
    "NN_add_pos": gemm_case(30, 264, 64, 64, 64, 264, "BF16_ADD_POS", bias=True, C2=True, aux=True, seg_rows=10),
    "NT_row_gather": gemm_case(25, 64, 64, 32, 32, 128, b_trans=1, rowmap=_rowmap_gaps_and_runs(25, 1, 1)),
    "NT_row_gather_gelu_z": gemm_case(25, 64, 64, 32, 32, 128, "MUL_GELU_GRAD_Z", b_trans=1, aux=True,
                                      rowmap=_rowmap_gaps_and_runs(25, 1, 2)),
    "TT_k_gather_atomic": gemm_case(32, 96, 40, 32, 64, 96, "ATOMIC_F32", a_trans=1, b_trans=1, split_k=2,
                                    rowmap=np.concatenate([_KG, np.zeros(256, np.int32)])),
    "fp8_bf16_bias": fp8_case(40, 264, 256),
    "fp8_bias_gelu2_q": fp8_case(20, 256, 256, "BIAS_GELU2", C2=True, q_out=True),
    "fp8_bias_gelu_q_only": fp8_case(20, 256, 256, "BIAS_GELU", C=False, q_out=True),
    "wgrad_problem": gr.wgrad_fields(0, 0, 0, 24, 40, 77),
}


def _gelu32(h):
    return 0.5 * h * (1.0 + torch.special.erf(h / math.sqrt(2.0)))


def _gelu1_32(h):
    return 0.5 * (1.0 + torch.special.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)


def quantize(x):
    """q bytes [M][N] and scale dwords [N/128][M] of a bf16 [M][N] region (wj_quantize_mxfp8's rule)"""
    M, N = x.shape
    q, e = gr.quantize_mxfp8_torch(x, M, N)
    out = torch.zeros((N // 128) * M, dtype=torch.int32)
    gr.pack_scales(e, M, out, 0)
    return q, out.view(N // 128, M)


def emulate(o: gr.Operands, bias_first: bool, split: int = 1) -> None:
    """What a kernel of this form writes: fp32 accumulation over k blocks of 32 (each block's product rounded once), bias first or
    last, one fp32 partial per K split added to a += output in split order, the header's rounding points."""
    f = o.f
    M, N, K = f["M"], f["N"], f["K"]
    ins = o.epi_inputs(0, M)
    bias = ins["bias"].float() if "bias" in ins else None
    kps = ((K + split - 1) // split + 63) // 64 * 64 if split > 1 else K
    parts = []
    for s0 in range(0, K, kps):
        acc = torch.zeros(M, N, dtype=torch.float32)
        if bias is not None and bias_first and s0 == 0:
            acc += bias
        for k0 in range(s0, min(K, s0 + kps), 32):
            k1 = min(K, k0 + 32, s0 + kps)
            acc += (o.a_block(0, M, k0, k1) @ o.b_block(k0, k1)).float()
        parts.append(acc)
    e = f["epilogue"]
    if e == "ATOMIC_F32":
        c = o.region("C").clone()
        for p in parts:
            c += f["alpha"] * p
        o.set_region("C", c)
        return
    acc = parts[0]
    if bias is not None and not bias_first:
        acc = acc + bias
    out = {}
    if e == "BF16":
        out["C"] = acc.to(torch.bfloat16)
    elif e == "ADD_F32":
        out["C"] = acc + ins["aux"].float()
    elif e in ("BIAS_GELU", "BIAS_GELU2"):
        h = acc.to(torch.bfloat16).float()
        g = _gelu32(h).to(torch.bfloat16)
        if e == "BIAS_GELU":
            out["C"] = g
        else:
            out["C"], out["C2"] = _gelu1_32(h).to(torch.bfloat16), g
    elif e == "MUL_GELU_GRAD":
        out["C"] = (acc.to(torch.bfloat16).float() * ins["aux"].float()).to(torch.bfloat16)
    elif e == "MUL_GELU_GRAD_Z":
        out["C"] = (acc.to(torch.bfloat16).float() * _gelu1_32(ins["aux"].float())).to(torch.bfloat16)
    elif e == "CONV_GELU":
        valid = ((torch.arange(M) % f["seg_rows"]) < f["seg_valid"])[:, None]
        pre = torch.where(valid, acc, torch.zeros_like(acc)).to(torch.bfloat16)
        out["C"], out["C2"] = pre, _gelu32(pre.float()).to(torch.bfloat16)
    elif e == "BF16_ADD_POS":
        y = acc.to(torch.bfloat16).float() + ins["aux"].float()
        out["C"], out["C2"] = y.to(torch.bfloat16), y
    if f["colsum"]:
        cs = o.b["colsum"]
        cs.t[cs.p:cs.p + N] += out["C"].float().sum(0)
    if f.get("q_out"):
        q, s = quantize(out["C2" if e == "BIAS_GELU2" else "C"])
        o.b["q_out"].rows(0, M, N, f["ldc"]).copy_(q)
        o.b["q_scales"].rows(0, N // 128, M, f["ld_q_scale"]).copy_(s)
    for n, v in out.items():
        if n in gr.out_dtypes(f):
            o.set_region(n, v)
    o.emulated = out


def run(name, bias_first=False):
    f = CASES[name]
    o = gr.Operands(f, "cpu", seed=5)
    o.reset_outputs()
    snap = o.snapshot()
    exp = gr.reference(o, snap)
    split = f["split_k"] if f["split_k"] > 1 else (3 if f["entry"] == "wgrad" else 1)
    emulate(o, bias_first, split)
    return o, exp, snap, split


@pytest.mark.parametrize("bias_first", [False, True])
@pytest.mark.parametrize("name", sorted(CASES))
def test_emulated_kernel_passes_every_check(name, bias_first):
    o, exp, snap, _ = run(name, bias_first)
    q_only = o.f.get("q_out") and not o.f["C"]
    fails, worst = gr.check(o, exp, snap, quantize=quantize, q_source=o.emulated["C"] if q_only else None)
    assert not fails, fails
    assert worst < 1.0 and (worst > 0.0 or not exp.ref)
    if o.f.get("q_out"):                     # a q_out that is not the quantised gelu(h) is rejected
        q = o.b["q_out"].t.clone()
        q[o.b["q_out"].p + 3] ^= 1
        outs = {n: o.b[n].t for n in snap}
        fails, _ = gr.check(o, exp, snap, dict(outs, q_out=q), quantize=quantize, q_source=o.emulated["C"] if q_only else None)
        assert any("q_out" in s for s in fails)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_mutation_is_rejected(name):
    o, exp, snap, split = run(name)
    outs = {n: o.b[n].t for n in snap}
    seen = []
    for what, mutated in gr.mutations(o, exp, outs, split):
        fails, _ = gr.check(o, exp, snap, mutated, quantize=quantize)
        assert fails, f"{name}: mutation '{what}' passed the check"
        seen.append(what)
    assert not exp.ref or (any("ulps" in s for s in seen) and any("k-slice" in s for s in seen))


def test_writes_outside_the_region_are_rejected():
    # one column past N (ldc > N)
    o, exp, snap, _ = run("NN_bf16_bias_N8_lda_ldc")
    f = o.f
    c = o.b["C"]
    t = c.t.clone()
    t[c.p + 5 * f["ldc"] + f["N"]] = 1.0
    fails, _ = gr.check(o, exp, snap, {"C": t})
    assert any("outside the output region" in s for s in fails)
    # behind the last row, into the guard band
    t = c.t.clone()
    t[c.p + (f["M"] - 1) * f["ldc"] + f["ldc"]] = 0.5
    assert any("outside the output region" in s for s in gr.check(o, exp, snap, {"C": t})[0])
    # a storage row the rowmap does not list (a gap), and the row behind its last entry
    for name in ("NT_row_gather", "NT_row_gather_gelu_z"):
        o, exp, snap, _ = run(name)
        f = o.f
        rm = set(f["rowmap"].tolist())
        gap = next(r for r in range(int(f["rowmap"].min()), int(f["rowmap"].max())) if r not in rm)
        for row in (gap, int(f["rowmap"].max()) + 1):
            t = o.b["C"].t.clone()
            t[o.b["C"].p + row * f["ldc"] + 3] = 0.25
            fails, _ = gr.check(o, exp, snap, {"C": t})
            assert any("outside the output region" in s for s in fails), (name, row)
    # a NaN left inside the region (a tile nobody wrote)
    o, exp, snap, _ = run("NN_conv_gelu_overlapping")
    t = o.b["C2"].t.clone()
    t[o.b["C2"].p + 2 * o.f["ldc"] + 1] = float("nan")
    assert any("outside the bound" in s for s in gr.check(o, exp, snap, {"C": o.b["C"].t, "C2": t})[0])


def test_colsum_increment_is_checked():
    o, exp, snap, _ = run("NN_mul_gelu_grad_colsum_N136")
    cs = o.b["colsum"]
    t = cs.t.clone()
    t[cs.p + 7] += 0.05 * float(exp.ref["C"][:, 7].abs().sum())
    fails, _ = gr.check(o, exp, snap, {"C": o.b["C"].t, "colsum": t})
    assert any(s.startswith("colsum") for s in fails)


@pytest.mark.parametrize("kappa,out_term", [(1e6, gr.BF16_ROUND), (gr.KAPPA, 2.0 ** -4)])
def test_a_loosened_bound_lets_mutations_through(monkeypatch, kappa, out_term):
    """The sensitivity tests above depend on the bound's size: with kappa = 1e6 or a 2^-4 output term the ulp moves pass."""
    monkeypatch.setattr(gr, "KAPPA", kappa)
    monkeypatch.setattr(gr, "BF16_ROUND", out_term)
    o, exp, snap, split = run("NN_bf16_bias_N8_lda_ldc")
    outs = {n: o.b[n].t for n in snap}
    passed = [w for w, m in gr.mutations(o, exp, outs, split) if not gr.check(o, exp, snap, m)[0]]
    assert "C moved off by ulps" in passed


def test_extents_of_overlapping_windows_and_gathers():
    f = CASES["NN_conv_gelu_overlapping"]
    ext = gr.extents(f)
    assert ext["A"][:2] == (0, (33 - 1) * 64 + 96) and ext["C"][:2] == (0, 32 * 40 + 32)
    f = CASES["TT_k_gather_atomic"]
    ext = gr.extents(f)
    rm = f["rowmap"]
    assert ext["A"][:2] == (int(rm.min()) * 32, int(rm.max()) * 32 + 32) and ext["B"][:2] == (0, int(rm.max()) * 64 + 96)
    f = CASES["NN_add_pos"]
    assert gr.extents(f)["aux"][:2] == (0, 10 * 264)


def test_placement_keeps_the_recorded_page_offset():
    o = gr.Operands(CASES["NN_bf16_bias_N8_lda_ldc"], "cpu", seed=1)
    align = dict(CASES["NN_bf16_bias_N8_lda_ldc"]["align"])
    for n in ("A", "B", "C"):
        assert o.b[n].ptr % gr.PAGE == align[n]


def test_every_header_epilogue_has_a_reference():
    assert set(gr.EPI) == gr.SUPPORTED_EPILOGUES
    f = dict(CASES["NN_bf16_bias_N8_lda_ldc"], epilogue="NEW_EPI")
    assert gr.unsupported(f)
    assert gr.unsupported(dict(CASES["NN_bf16_bias_N8_lda_ldc"], unknown=("new_field",)))
    assert gr.unsupported(dict(CASES["NT_row_gather"], a_trans=0, b_trans=0))
