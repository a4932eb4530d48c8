"""Partial training through the HIP engine (GPU only): frozen parameters (JEPA.freeze, requires_grad_(False)), feature_grad_mult and the
freeze_feature_extractor_updates schedule.

Model and draw: DEEP of tests/test_recompute_gpu.py (7 student layers of width 128, 5 predictor layers of width 64), 4 clips of 2.01 s,
the golden AudioSet masks, deterministic mode unless stated.  Frozen sets (tests/freeze_reference.py): A the conv stack; B the conv
stack, the front and student layers 0-2 (floor = student layer 3); C every bias and predictor layer 1 (partly frozen units plus one
whole layer); D everything but the predictor and the two mappers.  The reference is the oracle step with requires_grad_(False) on the
frozen names (tests/freeze_reference.py); bounds are the yardstick's (tests/parity_yardstick.py) and PARITY.md's 1e-5 for two
summation orders.  Every test prints its figures before it asserts."""
import os
import sys

import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import freeze_reference as FR
from tests import launch
from tests import parity_yardstick as Y
from tests.test_jepa_gpu import build, dev, group_of, masks, oracle_kw
from tests.test_prenorm_gpu import build_pre, patch_oracle
from tests.test_recompute_gpu import DEEP, N_CLIPS, bits

pytestmark = pytest.mark.gpu

SETS = FR.SETS
_CACHE = {}


def draw(golden_dir, seed=3):
    mset = masks(golden_dir, N_CLIPS)
    audio = torch.from_numpy(synth.synth_audio(N_CLIPS, 1, 32159, seed=seed)).to(torch.bfloat16).to(dev())
    return audio, mset


def model(patterns=(), ragged=True, deterministic=True, builder=build, **kw):
    """a fresh DEEP model, frozen BEFORE its engine exists"""
    m, P = builder(DEEP, **kw)
    frozen = m.freeze(*patterns) if patterns else []
    eng = m._ensure_engine()
    eng.ragged, eng.deterministic = ragged, deterministic
    return m, P, frozen


def step(m, golden_dir, seed=3):
    audio, mset = draw(golden_dir, seed)
    out = m(audio, *mset)
    out["loss"].backward()
    torch.cuda.synchronize()
    return bits(out["loss"].detach().float().reshape(1)), m._flat.g32.clone()


def unfrozen(golden_dir, ragged):
    """(loss bits, gradient buffer) of the unfrozen model's deterministic step on the draw, computed once per form"""
    if ("plain", ragged) not in _CACHE:
        m, _, _ = model((), ragged)
        _CACHE[("plain", ragged)] = step(m, golden_dir)
    return _CACHE[("plain", ragged)]


def slices(m, g):
    return {n: g[s.offset:s.offset + s.numel].view(s.shape) for n, s in m._flat.by_name.items()}


def group_rel(m, a, b, names):
    return Y.group_errors(slices(m, a), slices(m, b), names, group_of)


def oracle_tables(P, golden_dir, frozen, m_mult=1.0):
    audio, (ctx, tgt, vis) = draw(golden_dir)
    args = (audio, ctx.to(dev()), tgt.to(dev()), vis.to(dev()))
    _, gbf = FR.grads(P, *args, frozen=frozen, m=m_mult, mode="bf16", **oracle_kw(DEEP))
    _, g32 = FR.grads(P, *args, frozen=frozen, m=m_mult, mode="fp32", **oracle_kw(DEEP))
    return gbf, g32


class Recorder:
    """every C-ABI entry issued inside the block, with the fields that tell the launches apart"""

    def __init__(self, monkeypatch):
        self.mp, self.log = monkeypatch, []

    def __enter__(self):
        from wavjepa_amd import _abi
        self.real = real = _abi.call

        def call(name, a, stream, lab=False):
            fields = [getattr(a, f, None) for f in ("epilogue", "a_trans", "M", "N", "K", "x_is_bf16")]
            self.log.append((name,) + tuple(v if isinstance(v, int) else None for v in fields))      # (a grouped entry's M, N are arrays)
            return real(name, a, stream, lab=lab)
        self.mp.setattr(_abi, "call", call)
        return self

    def __exit__(self, *exc):
        from wavjepa_amd import _abi
        torch.cuda.synchronize()
        self.mp.setattr(_abi, "call", self.real)

    def names(self):
        return [e[0] for e in self.log]

    def count(self, *prefixes):
        return sum(1 for n in self.names() if n.startswith(prefixes))


CONV_BWD = ("wj_conv0_gn_gelu_bwd", "wj_conv0_ln_gelu_bwd", "wj_conv0", "wj_gelu_bwd_bf16", "wj_conv_weight_layout", "wj_conv_ln_gelu_bwd",
            "wj_zero_rows")


def backward_log(m, golden_dir, monkeypatch, seed=3):
    audio, mset = draw(golden_dir, seed)
    out = m(audio, *mset)
    torch.cuda.synchronize()
    with Recorder(monkeypatch) as rec:
        out["loss"].backward()
    return rec


# ------------------------------------------------------------------------------------------------------------ 1 + 2. parity
@pytest.mark.parametrize("ragged", [True, False], ids=["ragged", "dense"])
@pytest.mark.parametrize("key", list(SETS))
def test_frozen_step_against_the_oracle_and_the_unfrozen_step(golden_dir, key, ragged):
    m, P, frozen = model(SETS[key], ragged)
    loss, g = step(m, golden_dir)
    assert m._engine.ragged_step == ragged and frozen
    loss0, g0 = unfrozen(golden_dir, ragged)
    print(key, "ragged" if ragged else "dense", "loss bits frozen / unfrozen:", int(loss), int(loss0), flush=True)
    names = [n for n in J.trainable_names(P) if n not in set(frozen)]
    params = dict(m.named_parameters())
    gs = slices(m, g)
    left = [n for n in frozen if params[n].grad is not None or float(gs[n].abs().max()) != 0.0]
    # 2. the rest is untouched: the trainable gradients against the unfrozen model's (regrouped weight-gradient launches may pick
    # other split factors: PARITY.md's bound for two summation orders)
    apart = group_rel(m, g, g0, names)
    print(key, "trainable groups against the unfrozen step (relative L2):", apart, "frozen tensors with a gradient:", left[:5], flush=True)
    # 1. the oracle with requires_grad_(False) on the frozen names, yardstick form
    gbf, g32 = oracle_tables(P, golden_dir, frozen)
    got = {n: params[n].grad for n in names}
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(key, "grad yardstick (d_hip, d_orc, pair, ratio):", {k: tuple(round(v, 5) for v in r.values()) for k, r in table.items()}, flush=True)
    assert torch.equal(loss, loss0)                                      # the forward does not change
    assert not left
    assert all(params[n].grad is not None for n in names)
    assert bool(torch.isfinite(g).all()) and all(float(got[n].abs().max()) > 0 for n in names if got[n].numel() > 1)
    for grp, e in apart.items():
        assert e < 1e-5, (grp, e)
    Y.assert_grad_yardstick(table)


def test_freezing_after_the_engine_exists_and_by_hand_is_the_same_step(golden_dir):
    m, _, frozen = model(SETS["B"])
    _, g = step(m, golden_dir)
    late, _, _ = model(())
    step(late, golden_dir)                                               # a step with nothing frozen first
    params = dict(late.named_parameters())
    for n in frozen:
        params[n].requires_grad_(False)                                  # by hand
    _, g2 = step(late, golden_dir)
    print("frozen late, by hand: gradient buffer bit-equal to frozen before construction:", bool(torch.equal(bits(g), bits(g2))), flush=True)
    assert torch.equal(bits(g), bits(g2))
    assert all(params[n].grad is None for n in frozen)
    late.unfreeze("*")
    _, g3 = step(late, golden_dir)
    assert all(p.grad is not None for n, p in late.named_parameters() if n in late._flat.by_name)
    assert torch.equal(bits(g3), bits(unfrozen(golden_dir, True)[1]))


# ------------------------------------------------------------------------------------------------------------ 3. feature_grad_mult
@pytest.mark.parametrize("mult", [0.5, 0.1])
def test_feature_grad_mult_scales_the_conv_gradients_only(golden_dir, mult):
    m, P, _ = model((), feature_grad_mult=mult)
    loss, g = step(m, golden_dir)
    loss0, g0 = unfrozen(golden_dir, True)
    conv = [n for n in m._flat.by_name if n.startswith("extract_audio.")]
    rest = [n for n in m._flat.by_name if not n.startswith("extract_audio.")]
    a, b = slices(m, g), slices(m, g0)
    differ = [n for n in rest if not torch.equal(bits(a[n]), bits(b[n]))]
    scaled = {n: b[n] * mult for n in conv}
    err = Y.group_errors(a, scaled, conv, group_of)["extract_audio"]
    # the bound: what the helper's own bf16 GradMultiply shows against its fp32 one on this draw, yardstick form
    gbf, g32 = oracle_tables(P, golden_dir, (), mult)
    d_orc = Y.group_errors(gbf, g32, conv, group_of)["extract_audio"]
    exact = all(torch.equal(bits(a[n]), bits(scaled[n])) for n in conv)
    print("feature_grad_mult", mult, "tensors outside the conv stack that differ:", differ[:5], "conv gradients against m x unscaled:", err,
          "bit-exact:", exact, "oracle bf16 against fp32 with GradMultiply:", d_orc, flush=True)
    assert torch.equal(loss, loss0) and not differ
    if mult == 0.5:
        assert exact
    else:
        assert err < Y.GRAD_FACTOR * d_orc
    params = dict(m.named_parameters())
    table = Y.grad_yardstick({n: params[n].grad for n in conv}, gbf, g32, conv, group_of)
    print("feature_grad_mult", mult, "conv yardstick against the helper:", table, flush=True)
    Y.assert_grad_yardstick(table)


def test_feature_grad_mult_0_is_set_a(golden_dir, monkeypatch):
    zero, _, _ = model((), feature_grad_mult=0.0)
    a, _, _ = model(SETS["A"])
    log0, loga = backward_log(zero, golden_dir, monkeypatch), backward_log(a, golden_dir, monkeypatch)
    torch.cuda.synchronize()
    print("feature_grad_mult = 0: launches", len(log0.log), "set A:", len(loga.log), flush=True)
    assert log0.log == loga.log and log0.count(*CONV_BWD) == 0
    assert torch.equal(bits(zero._flat.g32), bits(a._flat.g32))
    assert all(p.grad is None for n, p in zero.named_parameters() if n.startswith("extract_audio."))


# ------------------------------------------------------------------------------------------------------------ 4. launch evidence
def test_launches_of_the_frozen_sets(golden_dir, monkeypatch):
    from wavjepa_amd import ops
    plain, _, _ = model(())
    base = backward_log(plain, golden_dir, monkeypatch)
    again, _, _ = model(())
    again.freeze("extract_audio.*", "*.bias")
    again.unfreeze("*")
    back = backward_log(again, golden_dir, monkeypatch)
    logs = {k: backward_log(model(SETS[k])[0], golden_dir, monkeypatch) for k in ("A", "B", "D")}
    attn = ("wj_attn_bwd", "wj_attn_stream_bwd")
    fig = {k: dict(launches=len(r.log), conv=r.count(*CONV_BWD), attn=r.count(*attn), wgrad=r.count("wj_wgrad_grouped"),
                   unmask=r.count("wj_unmask_rows_f32"), ln=r.count("wj_layernorm_bwd"), colsum_bf16=r.count("wj_colsum_bf16"))
           for k, r in dict(logs, plain=base).items()}
    print("backward launches:", fig, flush=True)
    assert back.log == base.log                                          # nothing frozen: the same list, entry for entry
    p = fig["plain"]
    assert p["conv"] > 0 and p["attn"] == DEEP["l_enc"] + DEEP["l_dec"]
    # A: no conv backward entry, no GEMM with a conv epilogue (GELU' of the layer below), everything else as it was
    a = logs["A"]
    conv_epi = [e for e in a.log if e[0] == "wj_gemm_bf16" and e[1] == ops.EPI_MUL_GELU_GRAD_Z]
    assert fig["A"]["conv"] == 0 and not conv_epi
    n = len(a.log) - 1                                                   # the parent's backward, cut in front of the conv stack ...
    assert a.log[:n] == base.log[:n] and a.log[n][0] == "wj_colsum_f32_group"      # ... and the last grouped fold
    # B: the student's backward runs layers 3 .. 6, no boundary launch, nothing of _frontend_bwd
    b = fig["B"]
    assert b["conv"] == 0 and b["attn"] == DEEP["l_dec"] + 4
    assert b["unmask"] == p["unmask"] - 1                                # (the cast of d(local features) into d_lf_b)
    assert b["ln"] == p["ln"] - 1 - 2 * 3                                # feature_norms and two norms of each of layers 0 .. 2
    assert b["colsum_bf16"] == p["colsum_bf16"] - 1 - 3                  # the mapper's bias; linear1.bias of layers 0 .. 2 (deterministic mode: a pass of its own)
    # D: no weight gradient for the student: the predictor's grouped launches and the two mappers' only
    d = fig["D"]
    assert d["attn"] == DEEP["l_dec"] and d["conv"] == 0
    assert d["wgrad"] == p["wgrad"] - (DEEP["l_enc"] + 1) // 2
    student_shapes = [e for e in logs["D"].log if e[0] == "wj_gemm_bf16" and e[2] == 1 and DEEP["d_enc"] in (e[3], e[4])
                      and not {e[3], e[4]} == {DEEP["d_enc"], DEEP["d_dec"]}]
    assert not student_shapes


# ------------------------------------------------------------------------------------------------------------ 5. optimiser steps
@pytest.mark.parametrize("key", ["A", "B"])
def test_three_optimiser_steps_leave_the_frozen_parameters_alone(golden_dir, key):
    from wavjepa_amd.trainer import StepRunner
    m, P, frozen = model(SETS[key], warmup_steps=3)
    P = {k: v.detach().clone() for k, v in P.items()}
    m.trainer.max_steps = 20
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    run = StepRunner(m)
    m._engine.deterministic = True
    flat = m._flat
    ctx, tgt, vis = masks(golden_dir, N_CLIPS)
    audio, _ = draw(golden_dir)
    start = dict(p32=flat.p32.clone(), p16=None, t32=flat.t32.clone())
    state, worst, norms = {}, 0.0, []
    for i in range(3):
        out = m.training_step((audio, ctx, tgt, vis), i)
        out["loss"].backward()
        run.reducer.wait()
        want_norm = float(torch.cat([flat.g32[lo:hi] for lo, hi in flat.ranges_of(set(flat.by_name) - set(frozen))]).double().norm())
        held = float(torch.cat([flat.g32[lo:hi] for lo, hi in flat.ranges_of(set(frozen))]).abs().max())
        run.optimizer.step()
        run.scheduler.step()
        m.global_step = i + 1
        if start["p16"] is None:
            m._engine.wait_optimizer()
            start["p16"] = flat.p16.clone()
        r = FR.train_step(P, state, i, (audio, ctx.to(dev()), tgt.to(dev()), vis.to(dev())), frozen, mode="bf16", warmup=3, total_steps=20,
                          ema=(0.9, 0.99, 10), **oracle_kw(DEEP))
        gn = float(run.optimizer.grad_norm())
        worst = max(worst, abs(float(out["loss"].detach()) - r["loss"]) / abs(r["loss"]))
        norms.append((gn, want_norm, r["grad_norm"], held))
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    print(key, "worst relative loss deviation:", worst, "(reported norm, norm of the trainable ranges, oracle's, frozen max):", norms, flush=True)
    moved, decayed = [], []
    for n in frozen:
        s = flat.by_name[n]
        sl = slice(s.offset, s.offset + s.numel)
        if not (torch.equal(bits(flat.p32[sl]), bits(start["p32"][sl])) and torch.equal(flat.p16[sl].view(torch.int16), start["p16"][sl].view(torch.int16))):
            moved.append(n)
        if float(flat.adam_m[sl].abs().max()) != 0.0 or float(flat.adam_v[sl].abs().max()) != 0.0:
            decayed.append(n)
    print(key, "frozen tensors that moved:", moved[:5], "with non-zero moments:", decayed[:5], flush=True)
    assert not moved and not decayed
    assert len(run.optimizer.param_groups) == 2 and run.optimizer.param_groups[-1]["lr"] == 0.0
    assert worst < 2e-3
    for gn, want, orc, held in norms:
        assert held == 0.0 and abs(gn - want) < 1e-5 * want and abs(gn - orc) < 3e-2 * orc, (gn, want, orc, held)
    sd = m.state_dict()
    for k in ("encoder.layers.5.linear1.weight", "teacher_encoder.layers.5.linear1.weight", "decoder.layers.1.linear2.weight"):
        assert Y.rel(sd[k], P[k]) < 2e-3, k
    for k in frozen:
        assert torch.equal(sd[k].cpu(), P[k].cpu()), k                   # (the oracle's frozen tensors did not move either)
    if key == "B":
        # the teacher of a frozen student tensor: three EMA applications toward a constant
        name = "encoder.layers.1.linear1.weight"
        s, t = flat.by_name[name], flat.tby_name["teacher_" + name]
        const = start["p32"][s.offset:s.offset + s.numel].double()
        want = start["t32"][t.offset:t.offset + t.numel].double()
        for i in range(3):
            r = J.ema_decay(i, 0.9, 0.99, 10)
            want = r * want + (1 - r) * const
        err = Y.rel(flat.t32[t.offset:t.offset + t.numel], want)
        print("teacher of a frozen student tensor after three EMA steps, relative L2 to the closed form:", err, flush=True)
        assert err < 1e-6


# ------------------------------------------------------------------------------------------------------------ 6. schedule
def runner_steps(m, golden_dir, monkeypatch, n):
    """n optimisation steps in StepRunner's order on one draw -> (the runner, per step the backward's recorded launches, per step the
    conv parameters behind it)"""
    from wavjepa_amd.trainer import StepRunner
    m.trainer.max_steps = 20
    run = StepRunner(m)
    m._engine.deterministic = True
    flat = m._flat
    conv = flat.ranges_of({k for k in flat.by_name if k.startswith("extract_audio.")})
    audio, mset = draw(golden_dir)
    logs, after = [], []
    for i in range(n):
        out = m.training_step((audio,) + tuple(mset), i)
        with Recorder(monkeypatch) as rec:
            out["loss"].backward()
        run.reducer.wait()
        run.optimizer.step()
        run.scheduler.step()
        m.global_step = i + 1
        m._engine.wait_optimizer()
        logs.append(rec)
        after.append(torch.cat([flat.p32[lo:hi] for lo, hi in conv]).clone())
    torch.cuda.synchronize()
    return run, logs, after


def test_freeze_feature_extractor_updates_releases_the_conv_stack(golden_dir, monkeypatch):
    m, _, _ = model((), warmup_steps=1, freeze_feature_extractor_updates=2)
    first = torch.cat([m._flat.p32[lo:hi] for lo, hi in m._flat.ranges_of({k for k in m._flat.by_name if k.startswith("extract_audio.")})]).clone()
    run, logs, after = runner_steps(m, golden_dir, monkeypatch, 4)
    # the lists to compare with: one step of set A and one of the unfrozen model, issued the same way on the same draw
    list_a = runner_steps(model(SETS["A"], warmup_steps=1)[0], golden_dir, monkeypatch, 1)[1][0].log
    list_plain = runner_steps(model((), warmup_steps=1)[0], golden_dir, monkeypatch, 1)[1][0].log
    counts = [r.count(*CONV_BWD) for r in logs]
    same = [(r.log == list_a, r.log == list_plain) for r in logs]
    print("conv backward launches per step:", counts, "(equals set A's list, equals the unfrozen list) per step:", same,
          "launches of A / unfrozen:", len(list_a), len(list_plain), "optimiser groups at the end:", len(run.optimizer.param_groups), flush=True)
    assert list_a != list_plain and counts[0] == counts[1] == 0 and counts[2] == counts[3] > 0
    assert same == [(True, False), (True, False), (False, True), (False, True)]      # steps 0-1 issue A's launches, steps 2-3 the parent's
    assert torch.equal(bits(after[1]), bits(first)) and not torch.equal(bits(after[2]), bits(first))
    assert len(run.optimizer.param_groups) == 1


def test_schedule_survives_checkpoint_and_resume_bit_for_bit(tmp_path):
    """Four steps straight against two steps, a checkpoint and a fresh start (differently initialised model, new optimiser and
    scheduler -- built while global_step is still 0, so with the lr = 0 group -- that resumes for the last two): the release at step 2
    is a function of global_step, so parameters, teacher and moments land on the same bits (deterministic mode)."""
    from wavjepa_amd.data import SyntheticAudioSource
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import Trainer

    def source():
        return SyntheticAudioSource(TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1), batch_size=2, samples_per_audio=2, n_tokens=200,
                                    seconds=3.0, seed=11, n_mask_sets=4, device=dev())
    mask_sets = source().mask_sets             # the masker draws from OS entropy (as upstream): one set of masks for both runs

    def loader(skip):
        src = source()
        src.mask_sets = mask_sets
        i = 0
        while True:
            b = src.next_batch()
            torch.manual_seed(1000 + i)        # the crop offsets of on_after_batch_transfer come from the global generator
            if i >= skip:
                yield b
            i += 1

    def run(seed, root, ckpt=None, skip=0):
        m, _ = build(DEEP, seed=seed, warmup_steps=2, freeze_feature_extractor_updates=2)
        tr = Trainer(max_steps=4, default_root_dir=str(root), checkpoint_every_n_steps=1, log_every_n_steps=0, deterministic=True)
        return m, tr.fit(m, train_dataloaders=loader(skip), ckpt_path=ckpt)

    ma, ra = run(7, tmp_path / "a")
    ck = tmp_path / "a" / "step=2.ckpt"
    saved = torch.load(ck, map_location="cpu", weights_only=False)
    assert saved["global_step"] == 2 and saved["hyper_parameters"]["freeze_feature_extractor_updates"] == 2
    conv = [k for k in saved["state_dict"] if k.startswith("extract_audio.")]
    init, _ = build(DEEP, seed=7, warmup_steps=2)
    held = all(torch.equal(saved["state_dict"][k].cpu(), init.state_dict()[k].cpu()) for k in conv)
    mb, rb = run(8, tmp_path / "b", ckpt=str(ck), skip=2)
    assert ma.global_step == mb.global_step == 4 and ra.optimizer._t == rb.optimizer._t == 4
    for m_ in (ma, mb):
        m_._engine.wait_optimizer()
    torch.cuda.synchronize()
    equal = {name: bool(torch.equal(bits(a), bits(b))) for name, a, b in (
        ("parameters", ma._flat.p32, mb._flat.p32), ("teacher", ma._flat.t32, mb._flat.t32), ("adam_m", ma._flat.adam_m, mb._flat.adam_m),
        ("adam_v", ma._flat.adam_v, mb._flat.adam_v))}
    moved = not all(torch.equal(ma.state_dict()[k].cpu(), saved["state_dict"][k].cpu()) for k in conv)
    print("straight run against checkpoint + resume, bit-equal:", equal, "conv tensors held through step 1:", held, "moved afterwards:", moved,
          "learning rates:", ra.scheduler.get_last_lr(), rb.scheduler.get_last_lr(), "groups:", len(ra.optimizer.param_groups),
          len(rb.optimizer.param_groups), flush=True)
    assert held and moved
    assert ra.scheduler.get_last_lr() == rb.scheduler.get_last_lr() and len(ra.optimizer.param_groups) == len(rb.optimizer.param_groups) == 1
    assert all(equal.values()), equal


# ------------------------------------------------------------------------------------------------------------ 7. options
def test_recomputation_with_a_floor_is_bit_equal(golden_dir):
    on, _, _ = model(SETS["B"], use_gradient_checkpointing=True)
    off, _, _ = model(SETS["B"])
    (l_on, g_on), (l_off, g_off) = step(on, golden_dir), step(off, golden_dir)
    print("set B, recomputation on / off: loss bits", int(l_on), int(l_off), "gradient bit-equal:", bool(torch.equal(bits(g_on), bits(g_off))), flush=True)
    assert on._engine.recompute and torch.equal(l_on, l_off) and torch.equal(bits(g_on), bits(g_off))


def test_layerdrop_takes_the_floor_over_the_kept_layers(golden_dir, monkeypatch):
    m, P, frozen = model(SETS["B"])
    m.layerdrop_keep = {"enc": [1, 4, 6]}
    rec = backward_log(m, golden_dir, monkeypatch)
    g = m._flat.g32.clone()
    ref, _, _ = model(())
    ref.layerdrop_keep = {"enc": [1, 4, 6]}
    _, g0 = step(ref, golden_dir)
    names = [n for n in m._flat.by_name if n not in set(frozen)]
    ran = [n for n in names if not n.startswith(("encoder.layers.0.", "encoder.layers.2.", "encoder.layers.3.", "encoder.layers.5."))]
    apart = group_rel(m, g, g0, ran)
    attn = rec.count("wj_attn_bwd", "wj_attn_stream_bwd")
    print("LayerDrop keep [1, 4, 6] with set B: attention backward launches", attn, "against the unfrozen LayerDrop step:", apart, flush=True)
    # the helper: the oracle walks layers 1, 4, 6 (tests/layerdrop_reference.py) with requires_grad_(False) on set B; the layers that
    # do not run get no gradient there either
    from tests import layerdrop_reference as LR
    LR.install(monkeypatch, {"enc": [1, 4, 6]})
    gone = [n for n in P if n in m._flat.by_name and n not in ran and n not in set(frozen)]
    gbf, g32 = oracle_tables(P, golden_dir, list(frozen) + gone)
    params = dict(m.named_parameters())
    table = Y.grad_yardstick({n: params[n].grad for n in ran}, gbf, g32, ran, group_of)
    print("LayerDrop keep [1, 4, 6] with set B, grad yardstick:", {k: tuple(round(v, 5) for v in r.values()) for k, r in table.items()}, flush=True)
    assert attn == DEEP["l_dec"] + 2                                     # student layers 4 and 6 only
    gs = slices(m, g)
    assert all(float(gs[n].abs().max()) == 0.0 for n in m._flat.by_name if n not in ran)
    for grp, e in apart.items():
        assert e < 1e-5, (grp, e)
    Y.assert_grad_yardstick(table)


def test_accumulation_of_two_micro_batches(golden_dir):
    m, _, frozen = model(SETS["A"])
    singles = []
    for seed in (3, 4):
        _, g = step(m, golden_dir, seed)
        singles.append(g.double())
    m.accumulate_grads = True
    opt = m.configure_optimizers()["optimizer"]
    opt.zero_grad()
    for seed in (3, 4):
        step(m, golden_dir, seed)
    got, want = m._flat.g32.clone(), singles[0] + singles[1]
    names = [n for n in m._flat.by_name if n not in set(frozen)]
    errs = group_rel(m, got.double(), want, names)
    held = max(float(slices(m, got)[n].abs().max()) for n in frozen)
    print("accumulation k = 2, set A, against two single backwards summed in fp64:", errs, "frozen max:", held, flush=True)
    with pytest.raises(ValueError, match="accumulation window"):
        m.unfreeze("extract_audio.*")
        audio, mset = draw(golden_dir)
        m(audio, *mset)
    m.freeze("extract_audio.*")
    assert held == 0.0
    for grp, e in errs.items():
        assert e < 1e-5, (grp, e)


def test_prenorm_with_a_floor_against_the_oracle(golden_dir, monkeypatch):
    m, P, frozen = model(SETS["B"], builder=build_pre)
    patch_oracle(monkeypatch)
    _, g = step(m, golden_dir)
    names = [n for n in J.trainable_names(P) if n not in set(frozen)]
    params = dict(m.named_parameters())
    gbf, g32 = oracle_tables(P, golden_dir, frozen)
    table = Y.grad_yardstick({n: params[n].grad for n in names}, gbf, g32, names, group_of)
    print("pre-norm, set B, grad yardstick:", {k: tuple(round(v, 5) for v in r.values()) for k, r in table.items()}, flush=True)
    gs = slices(m, g)
    assert all(float(gs[n].abs().max()) == 0.0 and params[n].grad is None for n in frozen)
    Y.assert_grad_yardstick(table)


def test_everything_frozen_launches_nothing_and_changes_nothing(golden_dir, monkeypatch):
    m, _, frozen = model(("*",))
    assert set(frozen) == set(m._flat.by_name)
    opt = m.configure_optimizers()["optimizer"]
    opt.max_grad_norm = 5.0
    rec = backward_log(m, golden_dir, monkeypatch)
    flat = m._flat
    flat.ensure_adam_state()
    before = [bits(t) for t in (flat.p32, flat.adam_m, flat.adam_v)] + [flat.p16.view(torch.int16).clone()]
    opt.step()
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    after = [bits(t) for t in (flat.p32, flat.adam_m, flat.adam_v)] + [flat.p16.view(torch.int16).clone()]
    print("everything frozen: backward launches", rec.names(), "gradient max", float(flat.g32.abs().max()), flush=True)
    assert rec.log == [] and float(flat.g32.abs().max()) == 0.0
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert all(p.grad is None for n, p in m.named_parameters())


# ------------------------------------------------------------------------------------------------------------ 8. never-written memory
def child_step(path):
    """(child process) one deterministic step of set B -> loss and gradient buffer at `path`"""
    import tests.conftest as C
    m, _, _ = model(SETS["B"])
    l, g = step(m, C.GOLDEN)
    torch.save({"loss": l.cpu(), "g32": g.cpu(), "fill": os.environ.get("WJ_ARENA_FILL", "")}, path)


def test_poisoned_arena_gives_the_same_step(golden_dir, tmp_path):
    """Every arena buffer filled with NaN before first use: a skipped producer whose consumer still runs would surface as a NaN or as
    other bits."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "poisoned.pt"
    code = f"import tests.conftest; from tests import test_freeze_gpu as T; T.child_step({str(path)!r})"
    rc, out, err = launch.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, WJ_ARENA_FILL="nan"), timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    got = torch.load(path, map_location="cpu", weights_only=False)
    assert got["fill"] == "nan"
    m, _, _ = model(SETS["B"])
    l, g = step(m, golden_dir)
    finite = bool(torch.isfinite(got["g32"]).all()) and bool(torch.isfinite(got["loss"].view(torch.float32)).all())
    print("set B, poisoned arena: finite", finite, "loss bits", int(got["loss"]), int(l), "gradient bit-equal",
          bool(torch.equal(bits(got["g32"]), bits(g.cpu()))), flush=True)
    assert finite
    assert torch.equal(got["loss"], l.cpu()) and torch.equal(bits(got["g32"]), bits(g.cpu()))


# ------------------------------------------------------------------------------------------------------------ 9. two ranks
def _worker(rank, world, port, golden_dir, q):
    import numpy as np
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [os.path.dirname(here), here, os.path.join(here, "golden")]
        from tests import test_accumulate_gpu as T
        from wavjepa_amd.ddp import section_ranges
        m, _ = T.fresh(warmup_steps=2)
        frozen = m.freeze(*SETS["A"])
        if rank == 1:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01)
        run = T.runner(m)
        assert run.reducer.active and run.sectioned and m._grads_ready_hook is not None
        flat = m._flat
        conv = flat.ranges_of(set(frozen))
        first = torch.cat([flat.p32[lo:hi] for lo, hi in conv]).clone()      # (behind the broadcast: rank 0's)
        fx = dict(np.load(os.path.join(golden_dir, "masks.npz")))
        launched, per_call = [0], []
        real_hook = run._hook

        def hook(tag):
            before = len(run.reducer.handles)
            real_hook(tag)
            launched[0] += len(run.reducer.handles) - before
        run._hook = m._grads_ready_hook = hook
        for i in range(3):
            lo = 2 * ((i + rank) % 3)
            batch = (T.clips(2, seed=300 + 2 * i + rank),) + tuple(torch.from_numpy(fx[k][lo:lo + 2]) for k in ("as_ctx", "as_tgt", "as_vis"))
            before = launched[0]
            out = run.step(batch, i)
            per_call.append(launched[0] - before)
        m._engine.wait_optimizer()
        torch.cuda.synchronize()
        buckets = sum(len(v) for v in section_ranges(flat, m.encoder.num_layers, run.reducer.enc_chunk).values())
        held = bool(torch.equal(bits(torch.cat([flat.p32[lo:hi] for lo, hi in conv])), bits(first)))
        sums = torch.stack([flat.p32.double().sum(), flat.p32.double().abs().sum(), flat.t32.double().sum()]).cpu()
        allsums = [torch.empty_like(sums) for _ in range(world)]
        dist.all_gather(allsums, sums)
        q.put((rank, per_call, buckets, held, [s.tolist() for s in allsums], float(out["loss"].detach())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_keep_their_collectives_and_the_frozen_tensors(golden_dir):
    import multiprocessing as mp

    import numpy as np
    from tests.test_accumulate_gpu import _free_port
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, golden_dir, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=560) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, per_call, buckets, held, allsums, loss in res:
        print("rank", rank, "collectives per step:", per_call, "buckets:", buckets, "frozen tensors bit-unchanged:", held, flush=True)
        assert buckets >= 3 and per_call == [buckets] * 3              # the collectives are what they were
        assert held
        assert allsums[0] == allsums[1], f"replicas diverged after three optimiser steps: {allsums}"
        assert np.isfinite(loss)


# ------------------------------------------------------------------------------------------------------------ 10. the launcher
@pytest.mark.parametrize("freeze", [True, False])
def test_launcher_freezes(tmp_path, freeze):
    import re

    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.size=tiny", "trainer.batch_size=1", "data.samples_per_audio=4",
           "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}", "seed=11"]
    if freeze:
        cmd.append("trainer.freeze=[extract_audio.*]")
    rc, out, err = launch.run(cmd, cwd=root, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    ck = torch.load(list(tmp_path.rglob("last.ckpt"))[0], map_location="cpu", weights_only=False)
    print("losses:", losses, "hyper-parameters beyond the usual:", sorted(set(ck["hyper_parameters"]) & {"freeze", "feature_grad_mult"}), flush=True)
    assert len(losses) == 3 and all(np.isfinite(losses))
    assert set(ck) == {"state_dict", "hyper_parameters", "global_step", "optimizer", "lr_scheduler"}
    if not freeze:
        assert not {"freeze", "feature_grad_mult", "freeze_feature_extractor_updates"} & set(ck["hyper_parameters"])
        return
    assert tuple(ck["hyper_parameters"]["freeze"]) == ("extract_audio.*",)
    # the conv tensors are the initial ones: the same seed builds the same model
    import train
    from wavjepa_amd.config import load_config
    cfg = load_config(os.path.join(root, "configs"), [c for c in cmd[2:] if not c.startswith("trainer.freeze")])
    torch.manual_seed(cfg.seed)                                          # (train.main's order: seed, trainer, model)
    train.setup_trainer(cfg)
    init, _ = train.build_model(cfg)
    conv = [k for k in init.state_dict() if k.startswith("extract_audio.")]
    moved = [k for k in conv if not torch.equal(init.state_dict()[k].cpu(), ck["state_dict"][k].cpu())]
    other = [k for k in ("encoder.layers.0.linear1.weight", "decoder.layers.0.linear1.weight") if torch.equal(init.state_dict()[k].cpu(), ck["state_dict"][k].cpu())]
    print("conv tensors that moved:", moved, "trained tensors that did not:", other, flush=True)
    assert conv and not moved and not other
