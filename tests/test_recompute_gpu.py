"""Activation recomputation (JEPA use_gradient_checkpointing=True -> EngineConfig.recompute) through the HIP engine (GPU only).

A deep small model -- 7 student and 5 predictor layers -- so that both rings of the backward (4 and 2 slots) wrap, at layer counts that
are no multiples of the ring sizes, across the student's weight-gradient group of 2, with the trimmed last predictor layer and the
bottom layer whose input is the stack's input.  The flag changes WHERE activations live and adds a second forward of every layer;
it must not change a bit of what is computed: in deterministic mode the loss and the gradient buffer are bit-equal with the flag
off, in default mode the loss is bit-equal and the gradient groups sit within the 1e-5 relative L2 that separates two summation
orders of the float atomics (PARITY.md, deterministic against default mode).  Oracle parity uses the yardstick forms and constants of
tests/parity_yardstick.py.  Every test prints its figures before it asserts."""
import gc
import os
import re
import sys

import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import launch
from tests import parity_yardstick as Y
from tests.test_attention_stream_gpu import drawn_masks
from tests.test_conv_layernorm_gpu import build_ln
from tests.test_jepa_gpu import ACT_TOL, GRAD_TOL, SMALL_SPEC, build, dev, group_of, masks, oracle_kw, rel
from tests.test_prenorm_gpu import _runner_steps, assert_activation_yardstick, build_pre, patch_oracle

pytestmark = pytest.mark.gpu

DEEP = dict(conv_spec=SMALL_SPEC, d_enc=128, h_enc=2, l_enc=7, d_dec=64, h_dec=2, l_dec=5, top_k=2)
DEEP_320 = dict(DEEP, conv_spec=SMALL_SPEC + [(64, 2, 2)])      # stride 320: 8.41 s = 420 tokens, above the whole-image attention kernels
N_CLIPS = 4

# form -> (builder, keyword arguments of the builder, engine attributes, clips, tokens, samples)
FORMS = {
    "post-ragged": (build, {}, {}, N_CLIPS, 200, 32159),
    "post-untrimmed": (build, {}, dict(trim_tail=False), N_CLIPS, 200, 32159),
    "post-dense": (build, {}, dict(ragged=False), N_CLIPS, 200, 32159),
    "pre-ragged": (build_pre, {}, {}, N_CLIPS, 200, 32159),
    "pre-dense": (build_pre, {}, dict(ragged=False), N_CLIPS, 200, 32159),
    "conv-layer-norm": (build_ln, {}, {}, N_CLIPS, 200, 32159),
    "dense-420-tokens": (build, dict(seconds=8.41, tokens=420), dict(ragged=False), 2, 420, 134560),
}


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def model(form, recompute, **kw):
    builder, bkw, attrs, _, tokens, _ = FORMS[form]
    cfg = DEEP_320 if tokens == 420 else DEEP
    m, P = builder(cfg, **dict(bkw, **kw), **(dict(use_gradient_checkpointing=True) if recompute else {}))
    eng = m._ensure_engine()
    assert eng.recompute == recompute and m.use_gradient_checkpointing == recompute
    for k, v in attrs.items():
        setattr(eng, k, v)
    return m, P, cfg


def draw(form, golden_dir, seed=3):
    _, _, _, n, tokens, samples = FORMS[form]
    mset = masks(golden_dir, n) if tokens == 200 else drawn_masks(n, tokens)
    audio = torch.from_numpy(synth.synth_audio(n, 1, samples, seed=seed)).to(torch.bfloat16).to(dev())
    return audio, mset


def one_step(form, golden_dir, recompute, deterministic):
    """a freshly built model's first forward + backward -> (loss bits, gradient buffer, model)"""
    m, _, _ = model(form, recompute)
    m._engine.deterministic = deterministic
    audio, mset = draw(form, golden_dir)
    out = m(audio, *mset)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert m._engine.ragged_step == FORMS[form][2].get("ragged", True)
    return bits(out["loss"].detach().float().reshape(1)), m._flat.g32.clone(), m


def differing(m, a, b):
    """names of the parameters whose slices of two gradient buffers differ in any bit"""
    out = []
    for name, sl in m._flat.by_name.items():
        if not torch.equal(bits(a[sl.offset:sl.offset + sl.numel]), bits(b[sl.offset:sl.offset + sl.numel])):
            out.append(name)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the same step
@pytest.mark.parametrize("form", list(FORMS))
def test_step_with_the_flag_is_bit_equal_in_deterministic_mode(golden_dir, form):
    l_on, g_on, m = one_step(form, golden_dir, True, True)
    l_off, g_off, _ = one_step(form, golden_dir, False, True)
    bad = differing(m, g_on, g_off)
    print(form, "loss bits on / off:", int(l_on), int(l_off), "gradient tensors that differ:", bad[:8], len(bad), flush=True)
    assert float(g_off.abs().max()) > 0 and bool(torch.isfinite(g_off).all())
    assert torch.equal(l_on, l_off)
    assert not bad and torch.equal(bits(g_on), bits(g_off))


@pytest.mark.parametrize("form", ["post-ragged", "pre-ragged"])
def test_step_with_the_flag_in_default_mode(golden_dir, form):
    l_on, g_on, m = one_step(form, golden_dir, True, False)
    l_off, g_off, _ = one_step(form, golden_dir, False, False)
    num, den = {}, {}
    for name, sl in m._flat.by_name.items():
        a, b = g_on[sl.offset:sl.offset + sl.numel].double(), g_off[sl.offset:sl.offset + sl.numel].double()
        grp = group_of(name)
        num[grp] = num.get(grp, 0.0) + float((a - b).pow(2).sum())
        den[grp] = den.get(grp, 0.0) + float(b.pow(2).sum())
    errs = {g: (num[g] / (den[g] + 1e-300)) ** 0.5 for g in num if den[g] > 0}
    print(form, "default mode, flag on against off: loss bits", int(l_on), int(l_off), "relative L2 per gradient group:", errs, flush=True)
    assert torch.equal(l_on, l_off)
    assert {"encoder", "decoder", "extract_audio"} <= set(errs)
    for g, e in errs.items():
        assert e < 1e-5, (g, e)


# ------------------------------------------------------------------------------------------------------------ 2. it recomputes
def stack_bytes(eng, stack):
    """bytes of the stack's activation buffers: every _Acts set (all layers, or the ring) and, in recompute mode, the kept outputs"""
    seen, total = set(), 0
    sets = getattr(eng, stack + "_acts")
    tensors = [getattr(a, name) for a in sets for name in type(a).__slots__]
    if eng.recompute:
        tensors += [t for pair in getattr(eng, stack + "_kept") for t in pair]
    for t in tensors:
        if t is not None and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


def stored_bytes(rows, D, H, B, T, layers):
    """what `layers` full activation sets take, from the shapes (engine._alloc_stack): per row qkv 3D, o, p, x1b, f, x2b D and h, g 4D
    in bf16, x1, x2 D in fp32, four fp32 row statistics; per (sequence, head, token) one fp32 log-sum-exp"""
    return layers * (rows * (2 * (3 * D + 5 * D + 8 * D) + 4 * 2 * D + 4 * 4) + 4 * B * H * T)


@pytest.mark.parametrize("pre", [False, True])
def test_activations_live_in_the_backward_rings(golden_dir, pre):
    form = "pre-ragged" if pre else "post-ragged"
    audio, mset = draw(form, golden_dir)
    peaks, engines = {}, {}
    for flag in (True, False):
        gc.collect()
        torch.cuda.empty_cache()
        m, _, _ = model(form, flag)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = m(audio, *mset)
        out["loss"].backward()
        torch.cuda.synchronize()
        peaks[flag] = torch.cuda.max_memory_allocated() - base
        engines[flag] = m._engine
        del out
    on, off = engines[True], engines[False]
    G = mset[1].shape[1]
    assert (on.cap_enc, on.cap_dec) == (off.cap_enc, off.cap_dec)
    assert len(on.enc_acts) == on.bw["enc"]["nbuf"] == 4 and len(on.dec_acts) == on.bw["dec"]["nbuf"] == 2
    assert len(off.enc_acts) == DEEP["l_enc"] and len(off.dec_acts) == DEEP["l_dec"]
    assert len(on.enc_kept) == DEEP["l_enc"] and len(on.dec_kept) == DEEP["l_dec"]
    for stack, rows, D, H, B, L in (("enc", on.cap_enc, DEEP["d_enc"], DEEP["h_enc"], N_CLIPS, DEEP["l_enc"]),
                                    ("dec", on.cap_dec, DEEP["d_dec"], DEEP["h_dec"], N_CLIPS * G, DEEP["l_dec"])):
        nbuf = on.bw[stack]["nbuf"]
        full = stored_bytes(rows, D, H, B, 200, L)
        bound = full * nbuf // L + 6 * D * rows * L
        got_on, got_off = stack_bytes(on, stack), stack_bytes(off, stack)
        print(form, stack, "rows", rows, "activation bytes off / on / bound:", got_off, got_on, bound, flush=True)
        assert got_off == full
        assert got_on <= bound and got_on < got_off
    print(form, "peak bytes allocated over one step, off / on:", peaks[False], peaks[True], flush=True)
    assert peaks[True] < peaks[False]


# ------------------------------------------------------------------------------------------------------------ 3. oracle parity
@pytest.mark.parametrize("form", ["post-ragged", "post-dense", "pre-ragged", "pre-dense"])
def test_oracle_parity_with_the_flag(golden_dir, monkeypatch, form):
    """The forms of test_forward_backward_parity on the deep model with the flag on: loss within 1e-3 relative of the oracle's bf16 flow,
    activations and gradient groups in the yardstick forms (tests/parity_yardstick.py, constants unchanged)."""
    if form.startswith("pre"):
        patch_oracle(monkeypatch)
    m, P, cfg = model(form, True)
    ragged = FORMS[form][2].get("ragged", True)
    audio, (ctx, tgt, vis) = draw(form, golden_dir)
    out = m(audio, ctx, tgt, vis)
    assert m._engine.ragged_step == ragged and m._engine.recompute
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(cfg))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(cfg))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    assert out["preds"].shape == ref["preds"].shape and out["preds"].dtype == torch.bfloat16
    preds = out["preds"].clone()
    if ragged:                                            # rows that were never visible read 0, as with the flag off
        assert float(preds[~seen].float().abs().max()) == 0.0
    lo, lr_, l32 = float(out["loss"]), float(ref["loss"]), float(ref32["loss"])
    print(form, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32, "rel", abs(lo - lr_) / abs(lr_), flush=True)
    assert_activation_yardstick(out, ref, ref32, seen, form)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    assert abs(lo - l32) < 2e-2 * abs(l32), (lo, l32)
    if form.startswith("post"):
        # the fixed regression bounds of test_forward_backward_parity for small batches (measured on post-norm activations of the small
        # model; the pre-norm tests use the yardstick forms alone)
        fixed = {k: rel(out[k].float(), ref[k].float()) for k in ("local_features", "contextual_features", "targets")}
        fixed["preds"] = rel(preds[seen].float(), ref["preds"][seen].float())
        print(form, "fixed bounds:", fixed, ACT_TOL["small"], flush=True)
        for k, bound in ACT_TOL["small"].items():
            assert fixed[k] < bound, (k, fixed[k], bound)
    out["loss"].backward()
    ref["loss"].backward()
    torch.cuda.synchronize()
    # the second forward (of the trimmed last predictor layer above all) left the predictions as the first wrote them
    assert torch.equal(m._engine.dense_preds().view(torch.int16), preds.view(torch.int16))
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gbf = {k: P[k].grad for k in names}
    assert set(names) <= set(got)
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(cfg))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(form, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()}, flush=True)
    Y.assert_grad_yardstick(table)
    if form.startswith("post"):
        for g, e in Y.group_errors(got, gbf, names, group_of).items():
            assert e < GRAD_TOL["small"], (g, e)


# ------------------------------------------------------------------------------------------------------------ 4. ring reuse
def wide_context(ctx, tgt):
    """the same targets with every other token as context: far more visible student rows than the golden masks have"""
    ctx2 = tgt.any(dim=1)                                   # [N, T] True = NOT context: only target positions stay hidden
    vis2 = (ctx2[:, None, :] & ~tgt).reshape(-1, tgt.shape[-1])
    return ctx2, tgt, vis2


@pytest.mark.parametrize("pre", [False, True])
def test_twenty_optimiser_steps_reuse_the_rings(golden_dir, pre):
    """20 optimiser steps in deterministic mode from the same state, flag on against off: parameters, Adam moments and losses bit for
    bit.  Steps 6-8 run 4 -> 3 -> 4 clips (the arena is rebuilt twice); step 12 has more visible student rows than the arena holds
    (it regrows); every step rewrites every ring slot twice while the side stream's weight gradients read the slots."""
    ctx, tgt, vis = masks(golden_dir, N_CLIPS)
    batches = []
    for i in range(20):
        n = 3 if i == 7 else N_CLIPS
        audio = torch.from_numpy(synth.synth_audio(n, 1, 32159, seed=900 + i)).to(torch.bfloat16).to(dev())
        mset = wide_context(ctx[:n], tgt[:n]) if i == 12 else (ctx[:n], tgt[:n], vis[:n])
        batches.append((audio,) + tuple(mset))
    ends, caps = {}, {}
    for flag in (True, False):
        m, _, _ = model("pre-ragged" if pre else "post-ragged", flag, warmup_steps=2)
        grown = []
        real = m._engine.alloc

        def alloc(*a, _real=real, _eng=m._engine, _grown=grown, **k):
            before = getattr(_eng, "cap_enc", 0), _eng.N
            _real(*a, **k)
            _grown.append((before, (_eng.cap_enc, _eng.N)))
        m._engine.alloc = alloc
        _, losses = _runner_steps(m, batches, deterministic=True)
        assert m._engine.recompute == flag and m._engine.ragged_step
        ends[flag] = (bits(losses), bits(m._flat.p32), bits(m._flat.adam_m), bits(m._flat.adam_v), bits(m._flat.t32))
        caps[flag] = grown
    (b11, n11), (a12, n12) = caps[True][11][1], caps[True][12][1]
    print("arena rows of the student before / after the wide step:", b11, a12, "clips per step:", [c[1][1] for c in caps[True]], flush=True)
    assert caps[True] == caps[False]
    assert [c[1][1] for c in caps[True]][5:9] == [4, 4, 3, 4] and a12 > b11 and n11 == n12 == 4
    assert int((~wide_context(ctx, tgt)[0]).sum()) > b11                   # the wide step's visible rows did not fit
    for name, a, b in zip(("losses", "parameters", "adam_m", "adam_v", "teacher"), ends[True], ends[False]):
        print(name, "bit-equal:", bool(torch.equal(a, b)), flush=True)
    for name, a, b in zip(("losses", "parameters", "adam_m", "adam_v", "teacher"), ends[True], ends[False]):
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(ends[True][1].view(torch.float32)).all())


# ------------------------------------------------------------------------------------------------------------ 5. never-written memory
def child_step(form, path):
    """(child process) one deterministic step with the flag on -> loss and gradient buffer at `path`"""
    import tests.conftest as C
    l, g, _ = one_step(form, C.GOLDEN, True, True)
    torch.save({"loss": l.cpu(), "g32": g.cpu(), "fill": os.environ.get("WJ_ARENA_FILL", "")}, path)


@pytest.mark.parametrize("form", ["post-ragged", "pre-ragged"])
def test_poisoned_arena_gives_the_same_step(golden_dir, tmp_path, form):
    """Every arena buffer filled with NaN before first use (WJ_ARENA_FILL=nan, read at import: a child process): a ring slot that the
    second forward rewrote only in part, or a kept output that was never written, would surface as a NaN or as other bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "poisoned.pt"
    code = f"import tests.conftest; from tests import test_recompute_gpu as R; R.child_step({form!r}, {str(path)!r})"
    rc, out, err = launch.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, WJ_ARENA_FILL="nan"), timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    got = torch.load(path, map_location="cpu", weights_only=False)
    assert got["fill"] == "nan"
    l, g, _ = one_step(form, golden_dir, True, True)
    finite = bool(torch.isfinite(got["g32"]).all()) and bool(torch.isfinite(got["loss"].view(torch.float32)).all())
    print(form, "poisoned arena: finite", finite, "loss bits", int(got["loss"]), int(l), "gradient bit-equal",
          bool(torch.equal(bits(got["g32"]), bits(g.cpu()))), flush=True)
    assert finite
    assert torch.equal(got["loss"], l.cpu()) and torch.equal(bits(got["g32"]), bits(g.cpu()))


# ------------------------------------------------------------------------------------------------------------ 6. the launcher
def test_launcher_trains_with_the_flag(tmp_path):
    """`train.py trainer.use_gradient_checkpointing=true trainer.size=tiny trainer.steps=3` in a child process: finite, moving losses and
    the flag in the checkpoint's hyper-parameters."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.use_gradient_checkpointing=true", "trainer.size=tiny", "trainer.batch_size=1",
           "data.samples_per_audio=4", "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    rc, out, err = launch.run(cmd, cwd=root, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    print("losses:", losses, flush=True)
    assert len(losses) == 3 and all(v == v and abs(v) < float("inf") for v in losses), out[-1500:]
    assert len(set(losses)) == 3
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    assert ck["hyper_parameters"].get("use_gradient_checkpointing") is True


# ------------------------------------------------------------------------------------------------------------ 7. fp8
def test_fp8_mode_is_refused_with_the_flag(golden_dir, monkeypatch):
    m, _, _ = model("post-ragged", True)
    m._engine.fp8 = True
    audio, mset = draw("post-ragged", golden_dir)
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*recomputation.*use_gradient_checkpointing"):
        m(audio, *mset)
    monkeypatch.setenv("WJ_FP8", "1")
    m2, _ = build(DEEP, use_gradient_checkpointing=True)
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*recomputation.*use_gradient_checkpointing"):
        m2._ensure_engine()
    monkeypatch.delenv("WJ_FP8")
    off, _, _ = model("post-ragged", False)            # (fp8 alone is still taken: the refusal is the combination's)
    off._engine.fp8 = True
    off._engine._check_fp8()
