"""Deterministic mode on the GPU: the store-and-sum forms of the weight gradients and column sums through the C ABI (fp64 bound of
tests/gemm_reference.py, bit-identical repeats under a concurrent load), and whole optimisation steps that must come out bit-identical
from run to run (loss, every gradient, parameters, Adam moments, checkpoints)."""
import gc
import os

import numpy as np
import pytest
import torch

import synth
from tests import gemm_reference as gr
from tests.test_deterministic_cpu import _group_split
from tests.test_jepa_gpu import BASE, SMALL, PinnedRng, build, group_of, masks

pytestmark = pytest.mark.gpu

REPEATS = 20


@pytest.fixture(scope="module")
def ops():
    from wavjepa_amd import ops as o
    o.require_gpu()
    return o


def dev():
    return torch.device("cuda:0")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


class Load:
    """An unrelated persistent GEMM kept running on a third stream while the launches under test repeat: it perturbs which workgroup
    finishes first, which is what the atomic forms' results depend on."""

    def __init__(self, ops):
        self.ops, self.stream = ops, torch.cuda.Stream()
        M, N, K = 16384, 1024, 1024
        g = torch.Generator(device=dev()).manual_seed(5)
        self.a = torch.randn(M, K, generator=g, device=dev()).to(torch.bfloat16)
        self.b = torch.randn(N, K, generator=g, device=dev()).to(torch.bfloat16)
        self.c = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
        self.dims = dict(M=M, N=N, K=K, lda=K, ldb=K, ldc=N)

    def kick(self, n=2):
        with torch.cuda.stream(self.stream):
            for _ in range(n):
                self.ops.gemm(self.a, self.b, self.c, schedule=4, **self.dims)


def _streams():
    return [torch.cuda.Stream(), torch.cuda.Stream()]


def _nan_ws(nbytes: int) -> torch.Tensor:
    return torch.full((max(nbytes, 256) // 4,), float("nan"), dtype=torch.float32, device=dev())


def _gemm_split(K, want):
    kps = gr._kps(K, max(1, want))
    return -(-K // kps)


def _replay_gemm_class(ops, f, seed, load, fails):
    o = gr.Operands(f, dev(), seed=seed)
    o.reset_outputs()                                  # C = random C_old inside the region, NaN outside
    snap = o.snapshot()
    exp = gr.reference(o, snap)
    need = ops.workspace_bytes("wj_gemm_bf16", M=f["M"], N=f["N"], K=f["K"], ldc=f["ldc"], a_trans=1, b_trans=1,
                               epilogue=gr.EPI["ATOMIC_F32"], split_k=f["split_k"], deterministic=1)
    split = _gemm_split(f["K"], f["split_k"])
    assert need == (split * f["M"] * f["ldc"] * 4 if split > 1 else 0), (need, split)
    ws = _nan_ws(need)
    first, worst = None, 0.0
    streams = _streams()
    for r in range(REPEATS):
        o.b["C"].t.copy_(snap["C"])
        ws.fill_(float("nan"))                          # no slab element may be read before it is written
        torch.cuda.synchronize()
        load.kick()
        with torch.cuda.stream(streams[r % 2]):
            ops.gemm(**o.kwargs(), workspace=ws, deterministic=True)
        torch.cuda.synchronize()
        if first is None:
            bad, worst = gr.check(o, exp, snap)
            fails += bad
            first = o.b["C"].t.clone()
            for what, mutated in gr.mutations(o, exp, {"C": first}, split):
                if not gr.check(o, exp, snap, mutated)[0]:
                    fails.append(f"mutation '{what}' was not rejected")
        elif not torch.equal(bits(o.b["C"].t), bits(first)):
            fails.append(f"launch {r}: {int((bits(o.b['C'].t) != bits(first)).sum())} elements of C differ from launch 0")
            break
    return split, worst, need


def _replay_group_class(ops, fs, seed, load, fails):
    os_ = [gr.Operands(f, dev(), seed=seed + i) for i, f in enumerate(fs)]
    snaps, exps = [], []
    for o in os_:
        o.reset_outputs()
        snaps.append(o.snapshot())
        exps.append(gr.reference(o, snaps[-1]))
    probs = [(o.b["A"].ptr, o.b["B"].ptr, o.b["C"].ptr, o.f["M"], o.f["N"], o.f["K"]) for o in os_]
    need = ops.wgrad_grouped_workspace_bytes(probs)
    ws = _nan_ws(need)
    # the launch's split per problem (launch_grouped's rule, mirrored in test_deterministic_cpu): the need is their slabs' sum
    shapes = [(f["M"], f["N"]) for f in fs]
    wide = all(n % 256 == 0 for _, n in shapes)
    m384 = all(m % 384 == 0 and n % 128 == 0 for m, n in shapes)
    tile = (256, 256, 256) if wide else ((384, 128, 256) if m384 else (256, 128, 512))
    splits = _group_split(shapes, [f["K"] for f in fs], *tile)
    assert need == (sum(s * m * n * 4 for s, (m, n) in zip(splits, shapes)) if max(splits) > 1 else 0), (need, splits)
    firsts, worst = None, 0.0
    streams = _streams()
    for r in range(REPEATS):
        for o, s in zip(os_, snaps):
            o.b["C"].t.copy_(s["C"])
        ws.fill_(float("nan"))
        torch.cuda.synchronize()
        load.kick()
        with torch.cuda.stream(streams[r % 2]):
            ops.wgrad_grouped(probs, workspace=ws, deterministic=True)
        torch.cuda.synchronize()
        if firsts is None:
            firsts = []
            for i, (o, e, s) in enumerate(zip(os_, exps, snaps)):
                bad, w = gr.check(o, e, s)
                worst = max(worst, w)
                fails += [f"problem {i}: {b}" for b in bad]
                firsts.append(o.b["C"].t.clone())
                for what, mutated in gr.mutations(o, e, {"C": firsts[-1]}, splits[i]):      # at this problem's own split
                    if not gr.check(o, e, s, mutated)[0]:
                        fails.append(f"problem {i}: mutation '{what}' was not rejected")
        else:
            for i, (o, f0) in enumerate(zip(os_, firsts)):
                if not torch.equal(bits(o.b["C"].t), bits(f0)):
                    fails.append(f"launch {r}, problem {i}: C differs from launch 0")
            if fails:
                break
    return worst, need


def test_weight_gradient_classes_of_the_benchmarked_step_in_deterministic_form(ops, monkeypatch):
    """Every weight-gradient call class of one 2s-bf16 training step at the benchmark's 256 clips (the grouped launches of predictor and
    student, the ungrouped col-form ATOMIC_F32 shapes, the sparse conv gather form with its recorded row list), replayed in the
    deterministic form: within the census test's per-element fp64 bound, its split mutations rejected, C += on a random C_old, a
    NaN-filled workspace before every launch, nothing outside C's region touched, and 20 launches on two alternating streams beside a
    persistent GEMM on a third bit-identical."""
    from tests.test_gemm_census_gpu import census, classes
    cls = classes(census(ops, monkeypatch, "2s-bf16", 256))
    wg = [(k, f, n) for k, f, n in cls if k == "wgrad" or (k == "gemm" and f["epilogue"] == "ATOMIC_F32")]
    assert any(k == "wgrad" for k, _, _ in wg) and any(k == "gemm" and f.get("rowmap") is not None for k, f, _ in wg)
    assert any(k == "gemm" and f.get("rowmap") is None for k, f, _ in wg)
    load = Load(ops)
    failing, split_seen = [], False
    for i, (kind, f, count) in enumerate(wg):
        fails = []
        if kind == "gemm":
            assert f["a_trans"] == 1 and f["b_trans"] == 1, gr.describe(f)
            split, worst, need = _replay_gemm_class(ops, f, 3000 + i, load, fails)
            split_seen = split_seen or split > 1
            line = f"x{count} {gr.describe(f)} | slices {split} | slab bytes {need} | max err/bound {worst:.3f}"
        else:
            worst, need = _replay_group_class(ops, f, 3000 + i, load, fails)
            split_seen = split_seen or need > 0
            line = "x%d wgrad_grouped [%s] | slab bytes %d | max err/bound %.3f" % (
                count, "; ".join(f"M={x['M']} N={x['N']} K={x['K']}" for x in f), need, worst)
        print(line + (" | FAIL" if fails else ""), flush=True)
        if fails:
            failing.append(line + "\n    " + "\n    ".join(fails[:8]))
        gc.collect()
        torch.cuda.empty_cache()
    assert split_seen
    assert not failing, f"{len(failing)} of {len(wg)} classes failed:\n" + "\n".join(failing)


def _relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _repeat_identical(launch, out_of, load):
    first = None
    streams = _streams()
    torch.cuda.synchronize()              # the operands were produced on the default stream; the launches go to streams of their own
    for r in range(REPEATS):
        load.kick(1)
        with torch.cuda.stream(streams[r % 2]):
            launch()
        torch.cuda.synchronize()
        got = [bits(t) for t in out_of()]
        if first is None:
            first = got
        else:
            for a, b in zip(got, first):
                assert torch.equal(a, b), f"launch {r} differs from launch 0 on {int((a != b).sum())} elements"


def test_column_sum_forms_are_bit_identical_and_match_fp32_torch(ops):
    load = Load(ops)
    g = torch.Generator(device=dev()).manual_seed(17)
    # wj_colsum_bf16: a bias gradient of the predictor (87 k rows x 1536) and the small shape of test_ops_gpu.test_colsum
    for M, N in ((87071, 1536), (1003, 192)):
        x = torch.randn(M, N, generator=g, device=dev()).to(torch.bfloat16)
        out = torch.empty(N, device=dev())
        ws = _nan_ws(ops.workspace_bytes("wj_colsum_bf16", M=M, N=N, deterministic=1))

        def launch():
            out.fill_(1.0)
            ws.fill_(float("nan"))
            ops.colsum_bf16(x, out, M=M, N=N, ldx=N, workspace=ws, deterministic=True)
        _repeat_identical(launch, lambda: [out], load)
        assert _relerr(out, 1 + x.float().sum(0)) < 1e-5
    # wj_colsum_f32 and the grouped fold: partial matrices of the size the LayerNorm / attention backward leave
    M, D = 1256, 768
    p = torch.randn(M, 3 * D, generator=g, device=dev())
    o1 = torch.empty(3 * D, device=dev())

    def launch_f32():
        o1.fill_(1.0)
        ops.colsum_f32(p, o1, M=M, N=3 * D, ldx=3 * D, deterministic=True)
    _repeat_identical(launch_f32, lambda: [o1], load)
    assert _relerr(o1, 1 + p.sum(0)) < 1e-5
    q = torch.randn(340, 1152, generator=g, device=dev())
    outs = [torch.empty(D, device=dev()) for _ in range(3)] + [torch.empty(1152, device=dev())]

    def launch_group():
        for t in outs:
            t.fill_(1.0)
        ops.colsum_f32_group([(p, 3 * D, M, 3 * D, outs[0], outs[1], outs[2], D), (q, 1152, 340, 1152, outs[3], None, None, 1152)],
                             deterministic=True)
    _repeat_identical(launch_group, lambda: outs, load)
    for i in range(3):
        assert _relerr(outs[i], 1 + p[:, i * D:(i + 1) * D].sum(0)) < 1e-5
    assert _relerr(outs[3], 1 + q.sum(0)) < 1e-5


@pytest.mark.parametrize("B,T,H,hd,ragged", [(64, 200, 12, 64, False), (48, 120, 12, 32, True), (8, 150, 4, 32, False), (4, 400, 12, 64, False),
                                             (6, 49, 4, 16, False)])
def test_attention_backward_bias_gradient_is_bit_identical(ops, B, T, H, hd, ragged):
    """wj_attn_bwd's dbias path in deterministic form (per-wave partials added in wave order, ordered fold): 20 launches identical,
    and = the column sums of its own dqkv within test_attention_fwd_bwd's bound; dqkv is the default form's, bit for bit."""
    load = Load(ops)
    D = H * hd
    g = torch.Generator(device=dev()).manual_seed(23)
    if ragged:
        lens = torch.randint(40, T + 1, (B,), generator=torch.Generator().manual_seed(3))
        off = torch.zeros(B + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0)
        rows, seq_off, lse_shape = int(off[-1]), off.to(dev()), (int(off[-1]), H)
    else:
        rows, seq_off, lse_shape = B * T, None, (B, H, T)
    qkv = torch.randn(rows, 3 * D, generator=g, device=dev()).to(torch.bfloat16)
    dout = torch.randn(rows, D, generator=g, device=dev()).to(torch.bfloat16)
    out = torch.empty(rows, D, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(lse_shape, device=dev())
    ops.attn_fwd(qkv, out, B=B, T=T, H=H, hd=hd, lse=lse, seq_off=seq_off)
    dqkv = torch.empty_like(qkv)
    dbias = torch.empty(3 * D, device=dev())
    ws = torch.empty(B, 3 * D, device=dev())

    def launch(det=True):
        dbias.fill_(1.0)
        ws.fill_(float("nan"))
        ops.attn_bwd(qkv, out, dout, lse, dqkv, B=B, T=T, H=H, hd=hd, dbias=dbias, dbias_ws=ws, seq_off=seq_off, deterministic=det)
    _repeat_identical(launch, lambda: [dbias, ws, dqkv], load)
    assert _relerr(dbias, 1 + dqkv.float().sum(0)) < 1e-4
    det_dqkv = bits(dqkv)
    launch(det=False)
    torch.cuda.synchronize()
    assert torch.equal(bits(dqkv), det_dqkv)
    assert _relerr(dbias, 1 + dqkv.float().sum(0)) < 1e-4


def _det_twin_cases():
    """(instantiation, hd, T, form) for every backward entry of the census module's BRANCHES at the first and last T of its range, in the
    forms it serves: key mask for the `true` frag kernels, none and ragged for the `false` ones, all three for the general kernel"""
    from tests.test_attention_census_gpu import BRANCHES
    cases = []
    for inst, (hd, lo, hi) in BRANCHES.items():
        if not inst.startswith("attn_bwd"):
            continue
        forms = ("mask",) if ", true" in inst else ("none", "ragged") if ", false" in inst else ("none", "ragged", "mask")
        cases += [(inst, hd, T, form) for T in (lo, hi) for form in forms]
    return cases


@pytest.mark.parametrize("inst,hd,T,form", _det_twin_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_every_deterministic_twin_of_the_backward_dispatch(ops, inst, hd, T, form):
    """The DET instantiation of every branch of wj_attn_bwd (B = 3, H = 2, random bf16 operands): dqkv equals the default launch's bit
    for bit; three deterministic launches agree bit for bit in dqkv, dbias_ws and dbias; dbias = the fp32 column sums of its own dqkv
    within the 1e-4 of test_attention_backward_bias_gradient_is_bit_identical."""
    from tests.test_attention_census_gpu import bwd_instantiation
    assert bwd_instantiation(dict(T=T, hd=hd, form=form)) == inst
    B, H = 3, 2
    D = H * hd
    g = torch.Generator(device=dev()).manual_seed(29)
    key_mask = seq_off = None
    rows, lse_shape = B * T, (B, H, T)
    if form == "ragged":
        lens = torch.tensor([T, max(1, T // 2), max(1, T - 1)])
        off = torch.zeros(B + 1, dtype=torch.int32)
        off[1:] = torch.cumsum(lens, 0)
        rows, seq_off, lse_shape = int(off[-1]), off.to(dev()), (int(off[-1]), H)
    elif form == "mask":
        m = torch.rand(B, T, generator=torch.Generator().manual_seed(T)) < 0.4
        m[:, T // 2] = False
        key_mask = m.to(torch.uint8).to(dev())
    qkv = torch.randn(rows, 3 * D, generator=g, device=dev()).to(torch.bfloat16)
    dout = torch.randn(rows, D, generator=g, device=dev()).to(torch.bfloat16)
    out = torch.empty(rows, D, dtype=torch.bfloat16, device=dev())
    lse = torch.empty(lse_shape, device=dev())
    ops.attn_fwd(qkv, out, B=B, T=T, H=H, hd=hd, lse=lse, seq_off=seq_off, key_mask=key_mask)
    dqkv = torch.empty_like(qkv)
    dbias = torch.empty(3 * D, device=dev())
    ws = torch.empty(B, 3 * D, device=dev())

    def launch(det):
        dqkv.fill_(float("nan"))
        dbias.fill_(1.0)
        ws.fill_(float("nan"))
        ops.attn_bwd(qkv, out, dout, lse, dqkv, B=B, T=T, H=H, hd=hd, dbias=dbias, dbias_ws=ws, seq_off=seq_off, key_mask=key_mask,
                     deterministic=det)
        torch.cuda.synchronize()
        return [bits(dqkv), bits(ws), bits(dbias)]
    default = launch(False)
    first = launch(True)
    assert torch.equal(first[0], default[0]), f"dqkv of the deterministic form differs from the default form's in {int((first[0] != default[0]).sum())} elements"
    for r in (1, 2):
        for name, a, b in zip(("dqkv", "dbias_ws", "dbias"), launch(True), first):
            assert torch.equal(a, b), f"deterministic launch {r} differs from launch 0 in {name}"
    assert not torch.isnan(dqkv.float()).any()
    assert _relerr(dbias, 1 + dqkv.float().sum(0)) < 1e-4


# ------------------------------------------------------------------------------------------------------------ whole steps
def _one_step(cfg, n, audio, mset, deterministic, ragged=True, sparse=True, seed=7, defer=True):
    """a freshly built model, one forward + backward + FusedAdamW.step; returns loss, gradients, parameters, Adam moments (as bits)"""
    m, _ = build(cfg, seed=seed, warmup_steps=2)
    eng = m._ensure_engine()
    eng.deterministic, eng.ragged, eng.sparse_conv = deterministic, ragged, sparse and eng.sparse_conv
    eng.defer_folds = defer and eng.defer_folds      # False: every fold at once (WJ_DEFER_FOLDS=0)
    m.trainer.max_steps = 10
    opt = m.configure_optimizers()["optimizer"]
    opt.max_grad_norm = 5.0
    out = m.training_step((audio,) + tuple(mset), 0)
    out["loss"].backward()
    assert eng.ragged_step == ragged
    torch.cuda.synchronize()
    grads = {k: bits(p.grad) for k, p in m.named_parameters() if p.grad is not None}
    gf = {k: p.grad.double().clone() for k, p in m.named_parameters() if p.grad is not None}
    opt.step()
    eng.wait_optimizer()
    torch.cuda.synchronize()
    res = dict(loss=bits(out["loss"].detach().float().reshape(1)), grads=grads, gf=gf, p=bits(m._flat.p32), m=bits(m._flat.adam_m),
               v=bits(m._flat.adam_v))
    del m, opt, out
    gc.collect()
    torch.cuda.empty_cache()
    return res


def _differing(runs):
    return sorted(k for k in runs[0]["grads"] if any(not torch.equal(r["grads"][k], runs[0]["grads"][k]) for r in runs[1:]))


@pytest.mark.parametrize("cfg_name,n,ragged,sparse,defer", [("base", 64, True, True, True), ("small", 4, False, True, True),
                                                            ("small", 4, True, False, True), ("small", 4, True, True, False)])
def test_four_fresh_models_take_the_same_step_bit_for_bit(golden_dir, cfg_name, n, ragged, sparse, defer):
    """Loss, EVERY trainable parameter's gradient (raw bits, tensor by tensor), and parameters and both Adam moments after
    FusedAdamW.step are identical across four freshly built models in deterministic mode."""
    cfg = BASE if cfg_name == "base" else SMALL
    mset = masks(golden_dir, n)
    audio = torch.from_numpy(synth.synth_audio(n, 1, 32159, seed=41)).to(torch.bfloat16).to(dev())
    runs = [_one_step(cfg, n, audio, mset, True, ragged, sparse, defer=defer) for _ in range(4)]
    assert len(runs[0]["grads"]) > 20
    for r in runs[1:]:
        assert torch.equal(r["loss"], runs[0]["loss"])
    diff = _differing(runs)
    assert not diff, f"{len(diff)} of {len(runs[0]['grads'])} gradient tensors differ between runs: {diff[:12]}"
    for key in ("p", "m", "v"):
        for i, r in enumerate(runs[1:]):
            assert torch.equal(r[key], runs[0][key]), (key, i + 1, int((r[key] != runs[0][key]).sum()))
    if cfg_name == "base":
        off = [_one_step(cfg, n, audio, mset, False, ragged, sparse) for _ in range(4)]
        print(f"for information: with the mode off {len(_differing(off))} of {len(off[0]['grads'])} gradient tensors differ across four runs")


@pytest.mark.parametrize("cfg_name,n", [("base", 64), ("small", 4)])
def test_deterministic_mode_computes_the_default_modes_gradient(golden_dir, cfg_name, n):
    """Same draw, mode on against mode off: the forward is shared (loss bit-equal); every gradient group within the 1e-5 relative L2
    that test_step_is_reproducible_and_sparse_conv_backward_equals_dense uses for 'same gradient, different summation order'."""
    cfg = BASE if cfg_name == "base" else SMALL
    mset = masks(golden_dir, n)
    audio = torch.from_numpy(synth.synth_audio(n, 1, 32159, seed=43)).to(torch.bfloat16).to(dev())
    on, off = _one_step(cfg, n, audio, mset, True), _one_step(cfg, n, audio, mset, False)
    assert torch.equal(on["loss"], off["loss"])
    num, den = {}, {}
    for k, g0 in off["gf"].items():
        grp = group_of(k)
        num[grp] = num.get(grp, 0.0) + float((on["gf"][k] - g0).pow(2).sum())
        den[grp] = den.get(grp, 0.0) + float(g0.pow(2).sum())
    errs = {grp: (num[grp] / (den[grp] + 1e-300)) ** 0.5 for grp in num}
    print("deterministic against default, relative L2 per gradient group:", errs)
    for grp, e in errs.items():
        assert e < 1e-5, (grp, e)


def test_oracle_yardstick_bounds_hold_in_deterministic_mode(golden_dir, monkeypatch, ops):
    """The parity tests of test_jepa_gpu.py (tests/parity_yardstick.py bounds against the oracle) with WJ_DETERMINISTIC=1, the way
    bench.py reaches the mode: base-64-True and one channel-extractor case."""
    from tests import test_jepa_gpu as TJ
    monkeypatch.setenv("WJ_DETERMINISTIC", "1")
    seen = []
    real = ops.wgrad_grouped

    def spy(problems, stream=None, **kw):
        seen.append(bool(kw.get("deterministic")))
        return real(problems, stream=stream, **kw)
    monkeypatch.setattr(ops, "wgrad_grouped", spy)
    TJ.test_forward_backward_parity(golden_dir, "base", 64, True)
    assert seen and all(seen), "the engine did not read WJ_DETERMINISTIC"
    del seen[:]
    TJ.test_forward_backward_parity_channel_extractor("own", True)
    assert seen and all(seen)


def test_checkpoint_resume_is_bit_exact_in_deterministic_mode(tmp_path):
    """test_trainer_checkpoint_resume_continues_the_same_trajectory with trainer.deterministic: 3 steps, save, a fresh start that loads
    the checkpoint, 3 more steps, against 6 uninterrupted steps on identical batches.  Parameters, Adam moments, EMA teacher and step
    counters are BIT-equal at steps 4 and 6 (the default mode's 1e-5 / 5e-3 tolerances absorb its atomics; here there are none)."""
    from wavjepa_amd.data import SyntheticAudioSource
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import Trainer

    def source():
        return SyntheticAudioSource(TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1), batch_size=2, samples_per_audio=2, n_tokens=200,
                                    seconds=3.0, seed=11, n_mask_sets=4, device=dev())

    with PinnedRng(777):
        mask_sets = source().mask_sets

    def loader(skip):
        src = source()
        src.mask_sets = mask_sets
        i = 0
        while True:
            b = src.next_batch()
            torch.manual_seed(1000 + i)
            if i >= skip:
                yield b
            i += 1

    def run(seed, root, ckpt=None, skip=0):
        m, _ = build(SMALL, seed=seed, warmup_steps=2)
        tr = Trainer(max_steps=6, default_root_dir=str(root), checkpoint_every_n_steps=1, log_every_n_steps=0, deterministic=True)
        r = tr.fit(m, train_dataloaders=loader(skip), ckpt_path=ckpt)
        assert m._engine.deterministic
        return m, r

    ma, ra = run(7, tmp_path / "a")
    ck = tmp_path / "a" / "step=3.ckpt"
    mb, rb = run(8, tmp_path / "b", ckpt=str(ck), skip=3)
    assert ma.global_step == mb.global_step == 6 and ra.optimizer._t == rb.optimizer._t == 6
    assert ra.scheduler.get_last_lr() == rb.scheduler.get_last_lr()
    for step in (4, 6):
        a = torch.load(tmp_path / "a" / f"step={step}.ckpt", map_location="cpu", weights_only=False)
        b = torch.load(tmp_path / "b" / f"step={step}.ckpt", map_location="cpu", weights_only=False)
        assert a["global_step"] == b["global_step"] == step and a["optimizer"]["step"] == b["optimizer"]["step"] == step
        assert a["optimizer"]["lr"] == b["optimizer"]["lr"] and a["lr_scheduler"] == b["lr_scheduler"]
        assert set(a["state_dict"]) == set(b["state_dict"])
        for k, va in a["state_dict"].items():
            assert torch.equal(va, b["state_dict"][k]), (step, k)
        for k in ("m", "v"):
            assert torch.equal(a["optimizer"][k], b["optimizer"][k]), (step, k)
    torch.cuda.synchronize()
    for name, a, b in (("student", ma._flat.p32, mb._flat.p32), ("teacher", ma._flat.t32, mb._flat.t32),
                       ("adam_m", ma._flat.adam_m, mb._flat.adam_m), ("adam_v", ma._flat.adam_v, mb._flat.adam_v)):
        assert torch.equal(a, b), name


def test_denoiser_training_steps_are_bit_reproducible():
    """Two runs of three Denoiser training steps in deterministic mode end with bit-equal parameters."""
    from tests.test_denoiser_gpu import build as build_denoiser
    clean = torch.from_numpy(synth.synth_audio(4, 1, 32159, seed=51)).to(torch.bfloat16).to(dev())
    gen = (clean.float() + 0.3 * torch.from_numpy(synth.synth_audio(4, 1, 32159, seed=52)).to(dev())).to(torch.bfloat16)
    ends = []
    for _ in range(2):
        den, _, _ = build_denoiser(alpha=0.3)
        den._ensure_engine().deterministic = True
        opt = den.configure_optimizers()["optimizer"]
        opt.param_groups[0]["lr"] = 1e-3
        for step in range(3):
            out = den.training_step((gen, clean), step)
            out["loss"].backward()
            opt.step()
        torch.cuda.synchronize()
        ends.append(({k: bits(v) for k, v in den.named_parameters() if v.requires_grad}, bits(out["loss"].detach().float().reshape(1))))
    (pa, la), (pb, lb) = ends
    assert torch.equal(la, lb)
    assert len(pa) > 10
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_train_py_deterministic_runs_write_identical_checkpoints(tmp_path):
    """`train.py trainer.deterministic=true trainer.size=tiny` twice for three steps: the tensor payloads of the two last.ckpt files
    (parameters, teacher, Adam moments) are byte-identical."""
    import sys
    from tests import launch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cks = []
    for tag in ("a", "b"):
        cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.deterministic=true", "trainer.size=tiny", "trainer.batch_size=1",
               "data.samples_per_audio=4", "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path / tag}"]
        rc, out, err = launch.run(cmd, cwd=root, timeout=300)
        assert rc == 0, (out[-1500:], err[-4000:])
        found = list((tmp_path / tag).rglob("last.ckpt"))
        assert len(found) == 1
        cks.append(torch.load(found[0], map_location="cpu", weights_only=False))
    a, b = cks
    assert a["global_step"] == b["global_step"] == 3
    assert set(a["state_dict"]) == set(b["state_dict"])
    for k, va in a["state_dict"].items():
        assert va.numpy().tobytes() == b["state_dict"][k].numpy().tobytes() if va.dtype != torch.bfloat16 else torch.equal(va, b["state_dict"][k]), k
    for k in ("m", "v"):
        assert a["optimizer"][k].numpy().tobytes() == b["optimizer"][k].numpy().tobytes(), k
