"""The norm / column-sum / target / loss reference helper (tests/norm_reference.py) on the host.

  * its fp64 references agree with torch float64 (autograd of F.layer_norm, F.instance_norm, the MSE expression, plain sums);
  * an fp32 numpy emulation that sums in the order the kernels document stays below MARGIN of every bound, on every input kind and
    every width the GPU test uses -- the margin of the bounds, measured on the reference side only and printed;
  * every mutation of the emulation's output is rejected wherever it applies, the unmutated output is accepted;
  * every field of the nine argument structs is handled by the reference or named in its exclusion list.
"""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import norm_reference as nr
from wavjepa_amd import _abi

MARGIN = 0.8
M_ROWS = 9
GROUP_CASES = [(15, 3), (25, 5), (26, 13), (403, 201), (410, 200)]
COLSUM_CASES = [(1, 8), (31, 72), (33, 200), (1003, 192), (4099, 64)]
MSE_CASES = [(1, 1, 1, 4), (2, 3, 37, 384), (3, 4, 50, 768), (2, 2, 33, 1000)]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------------------ torch float64
def test_references_agree_with_torch_float64():
    M, D, eps = 7, 36, 1e-5
    c = nr.ln_inputs("randn", M, D, 1, with_r=True)
    s = nr.add_f32(c["x"], c["r"]).requires_grad_(True)
    g, b = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    y = F.layer_norm(s, (D,), g, b, nr.f32eps(eps))
    dy = (c["dy"] + c["dy2"]).double()
    y.backward(dy)
    fw = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
    assert rel(fw["y_f32"][0], y.detach()) < 1e-12
    assert rel(fw["mean"][0], s.detach().mean(1)) < 1e-12
    assert rel(fw["rstd"][0], torch.rsqrt(s.detach().var(1, unbiased=False) + nr.f32eps(eps))) < 1e-12
    bw = nr.layernorm_bwd(c["dy"], c["dy2"], c["x"], c["r"], c["gamma"], eps)
    assert rel(bw["ds_f32"][0], s.grad) < 1e-12 and rel(bw["dgamma"][0], g.grad) < 1e-12 and rel(bw["dbeta"][0], b.grad) < 1e-12
    pb = nr.layernorm_pre_bwd(dy.float(), c["dres"], s.detach().float(), c["gamma"], eps)
    assert rel(pb["ds_f32"][0], s.grad + c["dres"].double()) < 1e-12
    # column sums and the += contract
    x = nr.colsum_input("cancel", 33, 8, 2)
    assert rel(nr.colsum(x, torch.ones(8))[0], 1 + x.double().sum(0)) < 1e-12
    o = nr.colsum_f32_group(x, 3, [torch.ones(3), None, torch.zeros(3)])
    assert o[1] is None and rel(o[0][0], 1 + x.double()[:, :3].sum(0)) < 1e-12 and rel(o[2][0][:2], x.double()[:, 6:].sum(0)) < 1e-12
    # group statistics
    gs = nr.group_stats(s.detach(), None, 3)
    assert rel(gs["total"][0][0, 0], s.detach()[:3].sum()) < 1e-12 and rel(gs["total"][0][2, 1], (s.detach()[6:] ** 2).sum()) < 1e-12
    # teacher targets
    B, T, Dm, K = 3, 5, 8, 3
    xs = nr.instnorm_layers(B, T * Dm, K, 3)
    want = torch.stack([F.instance_norm(x.double().reshape(B, T, Dm).transpose(1, 2)[None], eps=nr.f32eps(1e-5))[0].transpose(1, 2)
                        for x in xs]).mean(0).reshape(B, T * Dm)
    assert rel(nr.instnorm_mean(xs, 1e-5)["targets"][0], want) < 1e-12
    acc = None
    for x in xs:
        acc = nr.instnorm_accumulate(x, acc, 1.0 / K, 1e-5)["targets"][0]
    assert rel(acc, want) < 1e-7          # scale = float32(1 / 3)
    # the MSE expression of test_instnorm_and_mse
    B, G, T, Dm = 2, 3, 5, 8
    c = nr.mse_inputs(B, G, T, Dm, 4)
    pr = c["preds"].double().requires_grad_(True)
    mask = (c["tgt"].reshape(B, G, T) != 0)
    err = ((pr.view(B, G, T, Dm) - c["targets"].double()[:, None]) ** 2).mean(-1) * mask
    loss = err.sum() / (mask.sum().double() + nr.f32eps(1e-8))
    loss.backward()
    ref = nr.masked_mse(c["preds"], c["targets"], c["tgt"], B, G, T, Dm)
    assert rel(ref["loss"][0][0], loss.detach()) < 1e-12 and float(ref["loss"][0][1]) == float(mask.sum())
    assert rel(ref["dpreds"][0], nr.bf16(pr.grad)) < 1e-12


# ------------------------------------------------------------------------------------------------------------ margin
def ln_emulated(kind, M, D, seed, with_r, eps, x_bf16=False):
    c = nr.ln_inputs(kind, M, D, seed, with_r, x_bf16)
    fw = nr.emulate_ln_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
    dy = c["dy"] + c["dy2"]
    bw = nr.emulate_ln_bwd(dy, t(fw["s_f32"]), c["gamma"], fw["mean"], fw["rstd"], c["dres"])
    return c, fw, bw


def test_emulation_stays_below_the_margin_of_every_bound():
    w = collections.defaultdict(float)

    def hold(name, got, pair):
        w[name] = max(w[name], nr.worst(t(got) if isinstance(got, np.ndarray) else got, *pair))

    for D in nr.WIDTHS:
        for kind in nr.KINDS:
            for with_r, eps in ((False, 1e-6), (True, 1e-5)):
                c, fw, bw = ln_emulated(kind, M_ROWS, D, 7, with_r, eps, x_bf16=(D == 200))
                ref = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
                for k in ("s_f32", "y_f32", "y_bf16", "mean", "rstd"):
                    hold(k, fw[k], ref[k])
                rb = nr.layernorm_pre_bwd(c["dy"] + c["dy2"], c["dres"], t(fw["s_f32"]), c["gamma"], eps)
                for k in ("ds_f32", "ds_bf16", "dgamma", "dbeta"):
                    hold(k, bw[k], rb[k])
                hold("dbias", bw["dbias"], nr.dbias(t(bw["ds_bf16"])))
    for kind in ("randn", "offset"):
        for M, rows in GROUP_CASES:
            for D in (36, 384):
                v = nr.make_rows(kind, M, D, 11)
                gs = nr.group_stats(v.double(), None, rows)
                hold("group_stats", nr.emulate_group_stats(v.numpy(), rows, fma=True), gs["parts"])
                c = nr.ln_inputs(kind, M, D, 11, False)
                y = nr.emulate_ln_fwd(c["x"], None, c["gamma"], c["beta"], 1e-6)["y_f32"]
                ref = nr.layernorm_fwd(c["x"], None, c["gamma"], c["beta"], 1e-6)["y_f32"]
                hold("group_stats(y)", nr.emulate_group_stats(y, rows, fma=True), nr.group_stats(ref[0], ref[1], rows)["parts"])
    for kind in ("randn", "cancel"):
        for M, N in COLSUM_CASES:
            x = nr.colsum_input(kind, M, N, 12)
            hold("colsum_f32", nr.emulate_colsum(x, torch.ones(N)), nr.colsum(x, torch.ones(N)))
            hold("colsum_bf16", nr.emulate_colsum(x.to(torch.bfloat16), torch.ones(N)), nr.colsum(x.to(torch.bfloat16), torch.ones(N)))
    kappa = 0.0
    for (T, D), K in (((1, 4), 1), ((25, 164), 8), ((200, 768), 3)):
        B, TD = 3, T * D
        xs = nr.instnorm_layers(B, TD, K, 13)
        prev = None
        for x in xs:
            got = nr.emulate_instnorm_accumulate(x, prev, 1.0 / K, 1e-5)
            hold("instnorm_accumulate", got, nr.instnorm_accumulate(x, prev, 1.0 / K, 1e-5)["targets"])
            prev = t(got)
        stats = np.stack([nr.emulate_group_stats(x.reshape(B * T, D).numpy(), T, fma=True) for x in xs])
        ref = nr.instnorm_mean(xs, 1e-5)
        hold("instnorm_mean", nr.emulate_instnorm_mean(xs, stats, 1e-5), ref["targets"])
        kappa = max(kappa, float(ref["kappa"][0].max()))
    for B, G, T, D in MSE_CASES:
        for mask in ("mixed", "ones", "zeros"):
            c = nr.mse_inputs(B, G, T, D, 14, mask)
            got = nr.emulate_masked_mse(c["preds"], c["targets"], c["tgt"], B, G, T, D, 0.5, 3.0)
            ref = nr.masked_mse(c["preds"], c["targets"], c["tgt"], B, G, T, D, 0.5, 3.0)
            hold("mse loss", got["loss"], ref["loss"])
            hold("mse dpreds", got["dpreds"], ref["dpreds"])
    print()
    for k, v in w.items():
        print(f"emulation / bound  {k:22s} {v:.3f}")
    print(f"instnorm_mean kappa up to {kappa:.0f}")
    over = {k: v for k, v in w.items() if not v < MARGIN}
    assert not over, f"emulation above {MARGIN} of the bound: {over}"


# ------------------------------------------------------------------------------------------------------------ mutations
def test_mutations_are_rejected_on_the_emulation():
    n = 0
    for D in nr.WIDTHS:
        for kind in nr.KINDS:
            eps = 1e-5 if kind == "tiny" else 1e-6
            c, fw, bw = ln_emulated(kind, M_ROWS, D, 21, with_r=(D % 8 == 0), eps=eps)
            ref = nr.layernorm_fwd(c["x"], c["r"], c["gamma"], c["beta"], eps)
            got = {k: t(v) for k, v in fw.items()}
            for k in ("y_f32", "y_bf16", "mean", "rstd"):
                nr.check(got[k], *ref[k], what=f"{kind} D={D} {k}")
            for label, k, m in nr.ln_fwd_mutations(c, got, eps, kind):
                assert nr.rejected(m, *ref[k]), f"{kind} D={D}: {label} accepted"
                n += 1
            if kind not in ("randn", "offset"):
                continue
            rb = nr.layernorm_pre_bwd(c["dy"] + c["dy2"], c["dres"], got["s_f32"], c["gamma"], eps)
            gb = {k: t(v) for k, v in bw.items()}
            rb["dbias"] = nr.dbias(gb["ds_bf16"])
            for k in ("ds_f32", "ds_bf16", "dgamma", "dbeta", "dbias"):
                nr.check(gb[k], *rb[k], what=f"{kind} D={D} {k}")
            for label, k, m in nr.ln_bwd_mutations(gb, rb["_terms"], M_ROWS):
                assert nr.rejected(m, *rb[k]), f"{kind} D={D}: {label} ({k}) accepted"
                n += 1
    # column sums: a row missing, a row twice, a column routed to the neighbouring output
    for kind in ("randn", "cancel"):
        for M, N in COLSUM_CASES:
            x = nr.colsum_input(kind, M, N, 22)
            got, ref = t(nr.emulate_colsum(x)), nr.colsum(x)
            nr.check(got, *ref, what="colsum")
            assert nr.rejected(nr.mutate_colsum_row(got, x[M - 1], -1), *ref) and nr.rejected(nr.mutate_colsum_row(got, x[0], 1), *ref)
            n += 2
    x = nr.colsum_input("randn", 7, 600, 23)
    o = nr.colsum_f32_group(x, 200, [torch.zeros(200)] * 3)
    got = [t(nr.emulate_colsum(x[:, i * 200:(i + 1) * 200])) for i in range(3)]
    a, b = nr.mutate_route(got[0], got[1], float(got[0][-1]))
    nr.check(got[0], *o[0], what="o0")
    assert nr.rejected(a, *o[0]) and nr.rejected(b, *o[1])
    # group statistics: the last part dropped (where it holds rows)
    for M, rows in GROUP_CASES:
        v = nr.make_rows("offset", M, 36, 24)
        gs = nr.group_stats(v.double(), None, rows)
        parts = t(nr.emulate_group_stats(v.numpy(), rows, fma=True))
        nr.check(parts.double().sum(1), *gs["total"], what="group totals")
        if -(-rows // nr.SPLIT) * (nr.SPLIT - 1) < rows:
            assert nr.rejected(nr.mutate_drop_last_part(parts), *gs["total"]), f"group_rows={rows}: dropped part accepted"
            n += 1
    # masked MSE: count off by one, dpreds on a non-target row, truncation
    for B, G, T, D in MSE_CASES:
        c = nr.mse_inputs(B, G, T, D, 25)
        got = nr.emulate_masked_mse(c["preds"], c["targets"], c["tgt"], B, G, T, D)
        ref = nr.masked_mse(c["preds"], c["targets"], c["tgt"], B, G, T, D)
        nr.check(t(got["loss"]), *ref["loss"], what="loss")
        nr.check(t(got["dpreds"]), *ref["dpreds"], what="dpreds")
        assert nr.rejected(nr.mutate_count(t(got["loss"])), *ref["loss"])
        m = nr.mutate_dpreds_offrow(t(got["dpreds"]), ref["_on"][0])
        assert m is None or nr.rejected(m, *ref["dpreds"])
        n += 2
    assert n > 700


# ------------------------------------------------------------------------------------------------------------ coverage gate
def test_every_field_of_the_argument_structs_is_handled_or_excluded():
    for name, handled in nr.HANDLED.items():
        fields = {f for f, _ in _abi._STRUCT_FIELDS[name]}
        excluded = set(nr.EXCLUDED.get(name, {}))
        assert not (handled & excluded), name
        assert fields - handled - excluded == set(), f"{name}: fields without a reference or an exclusion: {sorted(fields - handled - excluded)}"
        assert (handled | excluded) - fields == set(), f"{name}: listed but not in the header: {sorted((handled | excluded) - fields)}"
    assert set(nr.EXCLUDED) <= set(nr.HANDLED)
    assert {k for v in nr.EXCLUDED.values() for k in v} == {"y_fp8", "y_fp8_scales", "ld_fp8_scale", "workgroups"}
