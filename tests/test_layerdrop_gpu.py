"""LayerDrop (JEPA encoder_layerdrop / decoder_layerdrop, model.layerdrop_keep) through the HIP engine (GPU only).

The DEEP model of tests/test_recompute_gpu.py -- 7 student layers of width 128, 5 predictor layers of width 64 -- on 4 clips of 2.01 s
with the golden AudioSet masks: seven and five layers make both rings of the backward (4 and 2 slots) wrap at counts that are no
multiples of them, across the student's weight-gradient group of 2.  Kept sets are pinned through model.layerdrop_keep where a test
is about an edge (top and bottom skipped, one layer, none) and drawn where it is about the draw.  The oracle walks the same layers
through tests/layerdrop_reference.py; parity uses the yardstick forms and constants of tests/parity_yardstick.py.  Deterministic mode
wherever bits are compared.  Every test prints its figures before it asserts."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import jepa_oracle as J
from tests import dropout_reference as R
from tests import launch
from tests import layerdrop_reference as LR
from tests import parity_yardstick as Y
from tests.test_accumulate_gpu import launch_trace, runner, state_bits
from tests.test_jepa_gpu import dev, group_of, masks, oracle_kw, rel
from tests.test_prenorm_gpu import assert_activation_yardstick, clips, patch_oracle
from tests.test_recompute_gpu import DEEP, FORMS, N_CLIPS, bits, draw, model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_ENC, L_DEC = DEEP["l_enc"], DEEP["l_dec"]
SEED = 20240607
# (student, predictor) kept sets; None: every layer.  Student [0, 2, 3, 6]; top and bottom skipped; one layer; none.  Predictor: top
# skipped (the trimmed tail moves to layer 3); one layer; none (then nothing of the loss depends on the student: its gradient is 0).
KEPT = {
    "s0236-p013": ([0, 2, 3, 6], [0, 1, 3]),
    "s12345-p4": ([1, 2, 3, 4, 5], [4]),
    "s3-pall": ([3], None),
    "snone-p013": ([], [0, 1, 3]),
    "sall-pnone": (None, []),
}


def keep_of(case):
    enc, dec = KEPT[case]
    return {s: v for s, v in (("enc", enc), ("dec", dec)) if v is not None}


def one_step(form, golden_dir, keep=None, recompute=False, deterministic=True, **kw):
    """a freshly built model's first forward + backward -> (loss bits, gradient buffer, model)"""
    m, _, _ = model(form, recompute, **kw)
    m._engine.deterministic = deterministic
    m.layerdrop_keep = keep
    audio, mset = draw(form, golden_dir)
    out = m(audio, *mset)
    out["loss"].backward()
    torch.cuda.synchronize()
    return bits(out["loss"].detach().float().reshape(1)), m._flat.g32.clone(), m


# ------------------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("case", list(KEPT))
@pytest.mark.parametrize("form", ["post-ragged", "post-dense", "post-untrimmed", "pre-ragged", "conv-layer-norm"])
def test_oracle_parity_with_pinned_kept_sets(golden_dir, monkeypatch, form, case):
    """One forward + backward.  Loss within 1e-3 relative of the oracle's bf16 flow over the same layers, every activation and every
    gradient group over the parameters of the layers that ran on the yardstick, every parameter of a skipped layer exactly 0.0.
    Without the feature the skipped layers' gradients are non-zero and the loss is the full model's."""
    if form.startswith("pre"):
        patch_oracle(monkeypatch)
    if form == "conv-layer-norm":
        from tests.test_conv_layernorm_gpu import patch_oracle as patch_oracle_ln
        patch_oracle_ln(monkeypatch)
    keep = keep_of(case)
    LR.install(monkeypatch, keep)
    m, P, cfg = model(form, False)
    m.layerdrop_keep = keep
    ragged = FORMS[form][2].get("ragged", True)
    audio, (ctx, tgt, vis) = draw(form, golden_dir)
    out = m(audio, ctx, tgt, vis)
    assert m._engine.ragged_step == ragged
    ran = dict(enc=keep.get("enc", list(range(L_ENC))), dec=keep.get("dec", list(range(L_DEC))))
    skipped = LR.skipped_names(P, keep)
    names = [k for k in J.trainable_names(P) if k not in skipped]
    assert len(skipped) == 12 * (L_ENC + L_DEC - len(ran["enc"]) - len(ran["dec"]))
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(cfg))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(cfg))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    assert out["preds"].shape == ref["preds"].shape and out["preds"].dtype == torch.bfloat16
    lo, lr_, l32 = float(out["loss"].detach()), float(ref["loss"].detach()), float(ref32["loss"])
    tag = f"{form} {case}"
    print(tag, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32, "rel", abs(lo - lr_) / abs(lr_), flush=True)
    assert_activation_yardstick(out, ref, ref32, seen, tag)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    out["loss"].backward()
    ref["loss"].backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    worst = max([float(got[k].abs().max()) for k in skipped] + [0.0])
    print(tag, "largest |gradient| over the", len(skipped), "parameters of skipped layers:", worst, flush=True)
    assert set(names) | set(skipped) <= set(got)
    for k in skipped:
        assert P[k].grad is None and float(got[k].abs().max()) == 0.0, k
    gbf = {k: P[k].grad for k in names}
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(cfg))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(tag, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()}, flush=True)
    Y.assert_grad_yardstick(table)
    assert bool(torch.isfinite(m._flat.g32).all()) and m.last_kept == ran
    if keep.get("dec") != []:                        # (an empty predictor: nothing of the loss depends on the student)
        assert float(got["encoder.norm.weight"].abs().max()) > 0
    # the kept set matters: the oracle over every layer is another function
    monkeypatch.undo()
    full = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio, *dm, mode="bf16",
                          **oracle_kw(cfg)) if form.startswith("post-") else None
    if full is not None:
        print(tag, "loss of the oracle over every layer:", float(full["loss"]), flush=True)
        assert abs(lo - float(full["loss"])) > 1e-3 * abs(lo)


# ------------------------------------------------------------------------------------------------------------ 2. skipped = absent
def test_a_skipped_predictor_layer_is_an_absent_one(golden_dir):
    """Predictor kept [0, 1, 3], the student whole, against a model whose predictor HAS three layers with those parameters and the same
    student and teacher: loss and every shared tensor of the gradient buffer bit-equal in deterministic mode."""
    from tests.test_jepa_gpu import build
    kept = [0, 1, 3]
    l5, g5, m5 = one_step("post-ragged", golden_dir, keep=dict(dec=kept))
    m3, _ = build(dict(DEEP, l_dec=len(kept)))
    sd5 = m5.state_dict()
    sd3 = {}
    for k in m3.state_dict():
        src = k
        if k.startswith("decoder.layers."):
            j = int(k.split(".")[2])
            src = ".".join(["decoder", "layers", str(kept[j])] + k.split(".")[3:])
        sd3[k] = sd5[src].clone()
    m3.load_state_dict(sd3)
    m3._ensure_engine().deterministic = True
    audio, mset = draw("post-ragged", golden_dir)
    out = m3(audio, *mset)
    out["loss"].backward()
    torch.cuda.synchronize()
    l3, g3 = bits(out["loss"].detach().float().reshape(1)), m3._flat.g32
    bad, shared = [], 0
    for k, s3 in m3._flat.by_name.items():
        src = k
        if k.startswith("decoder.layers."):
            src = ".".join(["decoder", "layers", str(kept[int(k.split(".")[2])])] + k.split(".")[3:])
        s5 = m5._flat.by_name[src]
        shared += 1
        if not torch.equal(bits(g3[s3.offset:s3.offset + s3.numel]), bits(g5[s5.offset:s5.offset + s5.numel])):
            bad.append(k)
    print("loss bits with layers 2, 4 skipped / absent:", int(l5), int(l3), "shared tensors:", shared, "that differ:", bad[:8], len(bad), flush=True)
    assert torch.equal(l5, l3) and not bad and shared == len(m3._flat.by_name)
    for i in (2, 4):
        s = m5._flat.by_name[f"decoder.layers.{i}.linear1.weight"]
        assert float(g5[s.offset:s.offset + s.numel].abs().max()) == 0.0
    assert float(g3.abs().max()) > 0 and bool(torch.isfinite(g3).all())


# ------------------------------------------------------------------------------------------------------------ 3. all kept = the parent
def test_all_kept_is_the_model_without_the_option(golden_dir):
    LT = launch_trace()
    audio, mset = draw("post-ragged", golden_dir)
    ends, traces = [], []
    for on in (True, False):
        m, _, _ = model("post-ragged", False, **(dict(encoder_layerdrop=0.3) if on else {}))
        m._engine.deterministic = True
        if on:
            m.layerdrop_keep = dict(enc=list(range(L_ENC)), dec=list(range(L_DEC)))
        m(audio, *mset)["loss"].backward()             # (first call: allocations and probes)
        with LT.Trace(m._engine) as tr:
            out = m(audio, *mset)
            out["loss"].backward()
        ends.append((bits(out["loss"].detach().float().reshape(1)), bits(m._flat.g32)))
        traces.append(tr.lines)
        assert (m.last_kept is not None) == on
    print("events of a traced step, every layer listed / without the option:", len(traces[0]), len(traces[1]), flush=True)
    assert traces[0] == traces[1] and len(traces[0]) > 50
    assert torch.equal(ends[0][0], ends[1][0]) and torch.equal(ends[0][1], ends[1][1])


# ------------------------------------------------------------------------------------------------------------ 4. launch count
@pytest.mark.parametrize("case", ["s0236-p013", "s3-pall", "snone-p013"])
def test_a_skipped_layer_issues_no_launch(golden_dir, monkeypatch, case):
    """Attention launches by their arguments: 64-wide heads are the student's (packed: seq_off) and the teacher's (dense), 32-wide the
    predictor's.  Forward and backward launches follow the kept counts; the teacher issues 7 whatever is kept."""
    from wavjepa_amd import _abi
    keep = keep_of(case)
    m, _, _ = model("post-ragged", False)
    m.layerdrop_keep = keep
    audio, mset = draw("post-ragged", golden_dir)
    m(audio, *mset)["loss"].backward()
    log, real = [], _abi.call

    def call(name, a, stream, lab=False):
        if name in ("wj_attn_fwd", "wj_attn_bwd"):
            log.append((name, int(a.hd), bool(a.seq_off)))
        else:
            log.append((name, 0, False))
        return real(name, a, stream, lab=lab)
    monkeypatch.setattr(_abi, "call", call)
    m(audio, *mset)["loss"].backward()
    torch.cuda.synchronize()
    monkeypatch.setattr(_abi, "call", real)
    assert m._engine.ragged_step
    n_enc, n_dec = len(m.last_kept["enc"]), len(m.last_kept["dec"])
    count = {key: log.count(key) for key in (("wj_attn_fwd", 64, True), ("wj_attn_fwd", 64, False), ("wj_attn_fwd", 32, True),
                                             ("wj_attn_bwd", 64, True), ("wj_attn_bwd", 32, True))}
    gemms = sum(1 for n, _, _ in log if n == "wj_gemm_bf16")
    print(case, "kept", n_enc, n_dec, "attention launches:", count, "GEMM launches:", gemms, flush=True)
    assert count[("wj_attn_fwd", 64, True)] == n_enc == count[("wj_attn_bwd", 64, True)]
    assert count[("wj_attn_fwd", 32, True)] == n_dec == count[("wj_attn_bwd", 32, True)]
    assert count[("wj_attn_fwd", 64, False)] == L_ENC
    assert sum(1 for n, _, _ in log if n in ("wj_attn_fwd", "wj_attn_bwd")) == 2 * (n_enc + n_dec) + L_ENC


# ------------------------------------------------------------------------------------------------------------ 5. recompute
def drawn_steps(m, batches, k=1):
    """optimiser steps through StepRunner on ready crops -> per micro-batch (loss bits, gradient buffer as the backward left it, kept)"""
    m.trainer.max_steps = 20
    run = runner(m, k if k > 1 else None)
    seen = []
    real = run._update

    def update():
        torch.cuda.synchronize()
        seen[-1] = seen[-1][:1] + (bits(m._flat.g32),) + seen[-1][2:]
        real()
    run._update = update
    for i, b in enumerate(batches):
        seen.append((None, None, None))
        out = run.step(b, i)
        seen[-1] = (int(bits(out["loss"].detach().float().reshape(1))), seen[-1][1], {s: list(v) for s, v in m.last_kept.items()})
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    return run, seen


def ld_model(form="post-ragged", recompute=False, p_enc=0.3, p_dec=0.3, seed=SEED, **kw):
    m, P, _ = model(form, recompute, encoder_layerdrop=p_enc, decoder_layerdrop=p_dec, warmup_steps=kw.pop("warmup_steps", 2), **kw)
    m.dropout_seed = seed
    m._engine.deterministic = True
    return m, P


def batches_of(golden_dir, n, first_seed):
    ctx, tgt, vis = masks(golden_dir, 8)
    out = []
    for i in range(n):
        lo = 2 * (i % 3)
        out.append((clips(N_CLIPS, seed=first_seed + i), ctx[lo:lo + N_CLIPS], tgt[lo:lo + N_CLIPS], vis[lo:lo + N_CLIPS]))
    return out


@pytest.mark.parametrize("form", ["post-ragged", "pre-ragged"])
def test_recompute_with_drawn_sets_is_bit_equal(golden_dir, form):
    batches = batches_of(golden_dir, 6, 820)
    runs = {}
    for flag in (True, False):
        m, _ = ld_model(form, flag)
        assert m._engine.recompute == flag
        _, runs[flag] = drawn_steps(m, batches)
        runs[flag] = (runs[flag], state_bits(m))
    kept = [s[2] for s in runs[True][0]]
    print(form, "kept per step:", [(len(k["enc"]), len(k["dec"])) for k in kept], flush=True)
    assert kept == [s[2] for s in runs[False][0]]
    assert kept == [dict(enc=LR.kept_set(SEED, i, "enc", L_ENC, 0.3), dec=LR.kept_set(SEED, i, "dec", L_DEC, 0.3)) for i in range(6)]
    assert any(len(k["enc"]) < L_ENC for k in kept) and any(len(k["dec"]) < L_DEC for k in kept)
    for i, (a, b) in enumerate(zip(runs[True][0], runs[False][0])):
        assert a[0] == b[0], ("loss", i)
        assert torch.equal(a[1], b[1]), ("g32", i)
    for name in runs[True][1]:
        assert torch.equal(runs[True][1][name], runs[False][1][name]), name


# ------------------------------------------------------------------------------------------------------------ 6. trajectory
def trajectory_seed(steps, k=1, p_enc=0.3, p_dec=0.2):
    """The first seed from SEED on under which, over the forwards of `steps` optimiser steps, each stack has a forward with a skipped layer
    and every layer runs at least once.  Host arithmetic on the generator: a condition on the input."""
    for seed in range(SEED, SEED + 1000):
        sets = [LR.kept_sets(seed, c, dict(enc=L_ENC, dec=L_DEC), dict(enc=p_enc, dec=p_dec)) for c in range(steps * k)]
        if (all(any(len(s[st]) < n for s in sets) and set().union(*[s[st] for s in sets]) == set(range(n))
                for st, n in (("enc", L_ENC), ("dec", L_DEC)))):
            return seed, sets
    raise AssertionError("no seed")


NAMED = ("encoder.layers.1.linear1.weight", "teacher_encoder.layers.1.linear1.weight", "extract_audio.cnn.2.0.weight")


def trajectory(golden_dir, monkeypatch, k, steps):
    seed, sets = trajectory_seed(steps, k)
    for st, n in (("enc", L_ENC), ("dec", L_DEC)):
        assert any(len(s[st]) < n for s in sets) and set().union(*[s[st] for s in sets]) == set(range(n))
    m, P = ld_model(p_enc=0.3, p_dec=0.2, seed=seed, warmup_steps=3)
    P = {k_: v.detach().clone() for k_, v in P.items()}
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    m.trainer.max_steps = 20
    run = runner(m, k if k > 1 else None)
    kept = {}
    LR.install(monkeypatch, kept)
    batches = batches_of(golden_dir, steps * k, 100)
    state, worst, window = {}, 0.0, []
    for i, b in enumerate(batches):
        out = run.step(b, i)
        assert m.last_kept == sets[i], (i, m.last_kept, sets[i])                 # call counter k * step + micro-batch
        window.append(((b[0],) + tuple(t.to(dev()) for t in b[1:]), float(out["loss"].detach()), sets[i]))
        if not run.closed:
            continue
        step = i // k
        r = LR.train_window(P, state, step, [w[0] for w in window], [w[2] for w in window], kept, mode="bf16", warmup=3, total_steps=20,
                            ema=(0.9, 0.99, 10), **oracle_kw(DEEP))
        gn = float(run.optimizer.grad_norm())
        print("step", step, "kept", [(len(w[2]["enc"]), len(w[2]["dec"])) for w in window], "losses hip / reference:",
              [w[1] for w in window], r["losses"], "grad norm:", gn, r["grad_norm"], flush=True)
        for (_, lo, _), lr_ in zip(window, r["losses"]):
            worst = max(worst, abs(lo - lr_) / abs(lr_))
        assert abs(gn - r["grad_norm"]) < 3e-2 * r["grad_norm"], (step, gn, r["grad_norm"])
        window = []
    print(f"k = {k}: worst relative loss deviation over {len(batches)} forwards:", worst, flush=True)
    assert worst < 2e-3
    assert m.global_step == steps
    sd = m.state_dict()
    for name in NAMED:
        print(name, rel(sd[name], P[name]), flush=True)
        assert rel(sd[name], P[name]) < 2e-3, name


def test_training_trajectory_with_drawn_sets_vs_reference(golden_dir, monkeypatch):
    """6 optimiser steps, p = 0.3 / 0.2, through StepRunner against tests/layerdrop_reference.py in the oracle's bf16 mode, with the bounds
    of test_training_trajectory_vs_oracle (loss 2e-3, gradient norm 3e-2, the three named parameters 2e-3)."""
    trajectory(golden_dir, monkeypatch, 1, 6)


# ------------------------------------------------------------------------------------------------------------ 8. accumulation
def test_accumulation_draws_per_micro_batch(golden_dir, monkeypatch):
    """k = 2: the micro-batches of step s draw with call counters 2 s and 2 s + 1 (asserted against the host function inside), and the
    windows match the reference within the bounds of test_training_trajectory_at_k_2_vs_reference."""
    trajectory(golden_dir, monkeypatch, 2, 3)


# ------------------------------------------------------------------------------------------------------------ 7. resume
def test_checkpoint_resume_continues_the_kept_sequence(golden_dir, tmp_path):
    """4 deterministic steps against 2 steps, a checkpoint, a fresh model with another seed that resumes, 2 more: parameters, teacher and
    both Adam moments bit for bit -- the kept set of step s comes from (dropout_seed, s), both of which the checkpoint holds."""
    from wavjepa_amd.trainer import Trainer
    batches = batches_of(golden_dir, 4, 860)

    def run(root, seed, ckpt=None, skip=0):
        m, _ = ld_model(seed=seed)
        m.on_after_batch_transfer = lambda batch, idx=0: batch
        tr = Trainer(max_steps=4, default_root_dir=str(root), checkpoint_every_n_steps=2, log_every_n_steps=0, deterministic=True)
        tr.fit(m, train_dataloaders=iter(batches[skip:]), ckpt_path=ckpt)
        return m
    ma = run(tmp_path / "a", SEED)
    ck = torch.load(tmp_path / "a" / "step=2.ckpt", map_location="cpu", weights_only=False)
    assert ck["hyper_parameters"]["dropout_seed"] == SEED and ck["hyper_parameters"]["encoder_layerdrop"] == 0.3
    mb = run(tmp_path / "b", SEED + 99, ckpt=str(tmp_path / "a" / "step=2.ckpt"), skip=2)
    assert ma.global_step == mb.global_step == 4 and mb.dropout_seed == SEED
    assert ma.last_kept == mb.last_kept == dict(enc=LR.kept_set(SEED, 3, "enc", L_ENC, 0.3), dec=LR.kept_set(SEED, 3, "dec", L_DEC, 0.3))
    assert any(len(LR.kept_set(SEED, s, "enc", L_ENC, 0.3)) < L_ENC for s in (2, 3))
    a, b = state_bits(ma), state_bits(mb)
    for name in a:
        print(name, "bit-equal after the resume:", bool(torch.equal(a[name], b[name])), flush=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name


# ------------------------------------------------------------------------------------------------------------ 9. with dropout
def test_dropout_with_layerdrop_against_the_oracle_with_the_same_masks(golden_dir, monkeypatch):
    """Dropout 0.1 and student kept [0, 2, 3, 6]: the oracle gets the masks of layers 0, 2, 3, 6 by their OWN indices (the helper's walker
    hands the layer's parameter prefix on), so a layer's element masks do not depend on which other layers were skipped."""
    from tests.test_dropout_gpu import P_DROP, build_drop, draw as drop_draw
    keep = dict(enc=[0, 2, 3, 6])
    m, P = build_drop(P_DROP, P_DROP)
    eng = m._ensure_engine()
    m.dropout_call, m.layerdrop_keep = 5, keep
    audio, (ctx, tgt, vis) = drop_draw(golden_dir)
    out = m(audio, ctx, tgt, vis)
    assert eng.ragged_step and eng._drop_now == dict(enc=P_DROP, dec=P_DROP) and m.last_kept["enc"] == keep["enc"]
    provider = R.EngineMasks(m._dropout_key(), 5, dict(enc=P_DROP, dec=P_DROP), dev(), plan=eng.plan, tail=eng.tail is not None)
    provider.n_layers = dict(enc=L_ENC, dec=L_DEC)
    R.install(monkeypatch, provider)
    LR.install(monkeypatch, keep)
    skipped = LR.skipped_names(P, keep)
    names = [k for k in J.trainable_names(P) if k not in skipped]
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(DEEP))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(DEEP))
    seen = tgt.reshape(-1, vis.shape[-1]).to(dev())
    lo, lr_ = float(out["loss"].detach()), float(ref["loss"].detach())
    print("dropout + layerdrop: loss hip/oracle-bf16:", lo, lr_, "rel", abs(lo - lr_) / abs(lr_), flush=True)
    assert_activation_yardstick(out, ref, ref32, seen, "dropout-layerdrop")
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    out["loss"].backward()
    ref["loss"].backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert all(float(got[k].abs().max()) == 0.0 for k in skipped) and len(skipped) == 36
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(DEEP))
    table = Y.grad_yardstick(got, {k: P[k].grad for k in names}, g32, names, group_of)
    print("grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()}, flush=True)
    Y.assert_grad_yardstick(table)


# ------------------------------------------------------------------------------------------------------------ 10. eval, inference
def test_eval_and_inference_never_drop(golden_dir):
    audio, mset = draw("post-ragged", golden_dir)
    outs = []
    for kw in (dict(encoder_layerdrop=0.5, decoder_layerdrop=0.5), {}):
        m, _, _ = model("post-ragged", False, **kw)
        m.dropout_seed = SEED
        m.eval()
        with torch.no_grad():
            out = m(audio, *mset)
            rep = m.get_audio_representation(audio, None)
        assert m.last_kept is None and m._engine._kept_now == {}
        outs.append((bits(out["loss"].float().reshape(1)), out["preds"].clone(), out["targets"].clone(), rep.clone()))
    assert len(LR.kept_set(SEED, 0, "enc", L_ENC, 0.5)) < L_ENC           # (a training forward of this model would have dropped)
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][3]).all())


# ------------------------------------------------------------------------------------------------------------ 11. two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, golden_dir, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), GLOO_SOCKET_IFNAME="lo")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        here = os.path.dirname(os.path.abspath(__file__))
        sys.path[:0] = [os.path.dirname(here), here, os.path.join(here, "golden")]
        from tests import test_layerdrop_gpu as T
        from wavjepa_amd.ddp import section_ranges
        from wavjepa_amd.trainer import StepRunner
        m, _ = T.ld_model()
        m._engine.deterministic = False
        if rank == 1:
            with torch.no_grad():
                for p in m.parameters():
                    p.add_(0.01)
        m.trainer.max_steps = 20
        run = StepRunner(m)
        assert run.reducer.active and run.sectioned and m._grads_ready_hook is not None
        flat = m._flat
        fx = dict(np.load(os.path.join(golden_dir, "masks.npz")))
        tags, real_hook = [], m._grads_ready_hook

        def hook(tag):
            tags[-1].append(tag)
            real_hook(tag)
        m._grads_ready_hook = hook
        kept, handles = [], []
        for i in range(3):
            lo = 2 * ((2 * i + rank) % 3)                              # ranks see different clips and masks
            batch = (T.clips(2, seed=300 + 2 * i + rank),) + tuple(torch.from_numpy(fx[k][lo:lo + 2]) for k in ("as_ctx", "as_tgt", "as_vis"))
            tags.append([])
            out = m.training_step(batch, i)
            out["loss"].backward()
            handles.append(len(run.reducer.handles))
            run.reducer.wait()
            run.optimizer.step()
            run.scheduler.step()
            m.global_step = i + 1
            kept.append({s: list(v) for s, v in m.last_kept.items()})
        m._engine.wait_optimizer()
        torch.cuda.synchronize()
        buckets = sum(len(v) for v in section_ranges(flat, m.encoder.num_layers, run.reducer.enc_chunk).values())
        sums = torch.stack([flat.p32.double().sum(), flat.p32.double().abs().sum(), flat.t32.double().sum()]).cpu()
        allsums = [torch.empty_like(sums) for _ in range(world)]
        dist.all_gather(allsums, sums)
        q.put((rank, kept, handles, buckets, tags, [s.tolist() for s in allsums], float(out["loss"].detach())))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_skip_the_same_layers(golden_dir):
    """Two ranks over gloo on one GPU, p = 0.3 drawn, three steps: both ranks report the same kept sets (the draw's key carries no rank),
    every step launches one collective per bucket as a step without LayerDrop does (the DEEP model: 6; the two-layer model of
    tests/test_ddp_gpu.py has 4), the listener hears every layer once in descending order, and the replicas stay identical."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, golden_dir, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=560) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [dict(enc=LR.kept_set(SEED, i, "enc", L_ENC, 0.3), dec=LR.kept_set(SEED, i, "dec", L_DEC, 0.3)) for i in range(3)]
    order = ["dec"] + [f"enc:{i}" for i in range(L_ENC - 1, -1, -1)] + ["front"]
    for rank, kept, handles, buckets, tags, allsums, loss in res:
        print("rank", rank, "kept:", kept, "collectives per step:", handles, "buckets:", buckets, flush=True)
        assert kept == want
        assert handles == [buckets] * 3 and buckets == 6
        assert tags == [order] * 3
        assert allsums[0] == allsums[1], f"replicas diverged after three steps: {allsums}"
        assert np.isfinite(loss)
    assert any(len(k["enc"]) < L_ENC for k in want)


# ------------------------------------------------------------------------------------------------------------ 12. never-written memory
def child_step(form, path):
    """(child process) one deterministic step with student [1, 2, 3, 4, 5] -> loss and gradient buffer at `path`"""
    import tests.conftest as C
    l, g, _ = one_step(form, C.GOLDEN, keep=dict(enc=[1, 2, 3, 4, 5]))
    torch.save({"loss": l.cpu(), "g32": g.cpu(), "fill": os.environ.get("WJ_ARENA_FILL", "")}, path)


@pytest.mark.parametrize("form", ["post-ragged", "pre-ragged"])
def test_poisoned_arena_gives_the_same_step(golden_dir, tmp_path, form):
    """Every arena buffer filled with NaN before first use (WJ_ARENA_FILL=nan, read at import: a child process): a ring slot or an
    activation set addressed by layer index instead of walk position would be read without having been written."""
    path = tmp_path / "poisoned.pt"
    code = f"import tests.conftest; from tests import test_layerdrop_gpu as T; T.child_step({form!r}, {str(path)!r})"
    rc, out, err = launch.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, WJ_ARENA_FILL="nan"), timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    got = torch.load(path, map_location="cpu", weights_only=False)
    assert got["fill"] == "nan"
    l, g, _ = one_step(form, golden_dir, keep=dict(enc=[1, 2, 3, 4, 5]))
    finite = bool(torch.isfinite(got["g32"]).all()) and bool(torch.isfinite(got["loss"].view(torch.float32)).all())
    print(form, "poisoned arena: finite", finite, "loss bits", int(got["loss"]), int(l), "gradient bit-equal",
          bool(torch.equal(bits(got["g32"]), bits(g.cpu()))), flush=True)
    assert finite
    assert torch.equal(got["loss"], l.cpu()) and torch.equal(bits(got["g32"]), bits(g.cpu()))


# ------------------------------------------------------------------------------------------------------------ 13. the launcher
@pytest.mark.parametrize("on", [True, False])
def test_launcher_trains_with_layerdrop(tmp_path, on):
    cmd = [sys.executable, os.path.join(ROOT, "train.py"), "trainer.size=tiny", "trainer.batch_size=1", "data.samples_per_audio=4",
           "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    if on:
        cmd.append("trainer.encoder_layerdrop=0.5")
    rc, out, err = launch.run(cmd, cwd=ROOT, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    print("losses:", losses, re.findall(r"kept \d+/\d+", out), flush=True)
    assert len(losses) == 3 and all(np.isfinite(losses)), out[-1500:]
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    assert set(ck) == {"state_dict", "hyper_parameters", "global_step", "optimizer", "lr_scheduler"}
    hp = ck["hyper_parameters"]
    if on:
        assert hp["encoder_layerdrop"] == 0.5 and "dropout_seed" in hp and "decoder_layerdrop" not in hp
        assert len(re.findall(r"kept \d+/2", out)) == 3
    else:
        from tests.test_recompute_cpu import DEFAULT_HPARAMS, plain_path
        assert not {"encoder_layerdrop", "decoder_layerdrop", "dropout_seed"} & set(hp) and not re.findall(r"kept \d+/\d+", out)
        if plain_path():
            assert set(hp) == DEFAULT_HPARAMS


# ------------------------------------------------------------------------------------------------------------ 14. refusals
def test_fp8_mode_is_refused_with_layerdrop(golden_dir, monkeypatch):
    from tests.test_jepa_gpu import build
    m, _, _ = model("post-ragged", False, encoder_layerdrop=0.1)
    m._engine.fp8 = True
    audio, mset = draw("post-ragged", golden_dir)
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*layerdrop"):
        m(audio, *mset)
    monkeypatch.setenv("WJ_FP8", "1")
    m2, _ = build(DEEP, decoder_layerdrop=0.2)
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*layerdrop"):
        m2._ensure_engine()
    monkeypatch.delenv("WJ_FP8")
    off, _, _ = model("post-ragged", False)            # (fp8 alone is still taken: the refusal is the combination's)
    off._engine.fp8 = True
    off._engine._check_fp8()
    off.layerdrop_keep = dict(enc=[0])                 # ... and a pinned kept set on a model whose rates are 0 is refused at the step
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*layerdrop"):
        off(audio, *mset)
