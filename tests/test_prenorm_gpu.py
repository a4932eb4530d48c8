"""End-to-end parity of PRE-norm stacks (TransformerLayerCFG norm_first=True) through the HIP engine against the oracle (GPU only).

The oracle becomes a pre-norm oracle by replacing its layer function (tests/prenorm_reference.py, pinned to
torch.nn.TransformerEncoder(norm_first=True) by tests/test_prenorm_cpu.py).  Bounds are the yardstick forms of
tests/parity_yardstick.py with the project's constants -- d(HIP, fp32) against d(oracle-bf16, fp32) on the same draw -- not the
fixed ACT_TOL / GRAD_TOL tables of tests/test_jepa_gpu.py, which were measured on post-norm activations.

Trimmed predictor tail: the pre-norm predictor supports it (after the last layer's attention only the target rows go on), so on a
ragged step `preds` exist on the target rows, on a dense step on every row -- the rule of test_forward_backward_parity.
"""
import os
import sys

import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import launch
from tests import parity_yardstick as Y
from tests import prenorm_reference as R
from tests.test_jepa_gpu import BASE, SMALL, build, dev, group_of, masks, oracle_kw, rel

pytestmark = pytest.mark.gpu

LAYOUTS = {"both": (True, True), "dec": (False, True), "enc": (True, False)}     # (student + teacher, predictor) pre-norm


def build_pre(cfg, layout="both", **kw):
    """tests.test_jepa_gpu.build with norm_first set in the layer configs it creates (the student's is the d_enc-wide one)."""
    from wavjepa_amd import types as WT
    enc, dec = LAYOUTS[layout]
    saved, orig = WT.TransformerLayerCFG.__dict__["create"], WT.TransformerLayerCFG.create

    def create(**k):
        first = enc if k.get("d_model", 768) != cfg["d_dec"] else dec
        return orig(**dict(k, norm_first=first))
    WT.TransformerLayerCFG.create = staticmethod(create)
    try:
        m, P = build(cfg, **kw)
    finally:
        WT.TransformerLayerCFG.create = saved
    assert (m.encoder.norm_first, m.teacher_encoder.norm_first, m.decoder.norm_first) == (enc, enc, dec)
    return m, P


def patch_oracle(monkeypatch, layout="both"):
    enc, dec = LAYOUTS[layout]
    fn = R.pre_norm_layer if (enc and dec) else R.mixed_layer((R.STUDENT_TEACHER if enc else ()) + (R.PREDICTOR if dec else ()))
    monkeypatch.setattr(J, "post_norm_layer", fn)


def clips(n, seed=3):
    return torch.from_numpy(synth.synth_audio(n, 1, 32159, seed=seed)).to(torch.bfloat16).to(dev())


def assert_activation_yardstick(out, ref, ref32, seen, tag):
    report = {k: rel(out[k].float(), ref[k].float()) for k in ("local_features", "contextual_features", "targets")}
    report["preds"] = rel(out["preds"][seen].float(), ref["preds"][seen].float())
    to32 = {k: (rel(out[k].float(), ref32[k].float()), rel(ref[k].float(), ref32[k].float()))
            for k in ("local_features", "targets", "contextual_features")}
    to32["preds"] = (rel(out["preds"][seen].float(), ref32["preds"][seen].float()), rel(ref["preds"][seen].float(), ref32["preds"][seen].float()))
    print(tag, "rel errors vs oracle bf16:", report, "distance from the fp32 oracle (HIP, oracle-bf16):", to32)
    for k, (d_hip, d_orc) in to32.items():
        assert d_hip < Y.ACT_FACTOR * d_orc + Y.ACT_EPS, (k, d_hip, d_orc)
        assert report[k] < Y.PAIR_FACTOR * d_orc + Y.ACT_EPS, (k, report[k], d_orc)


@pytest.mark.parametrize("layout,cfg_name,n,ragged", [("both", "small", 4, True), ("both", "small", 4, False), ("both", "small", 1, True),
                                                      ("both", "base", 2, True), ("both", "base", 2, False),
                                                      ("dec", "small", 4, True), ("enc", "small", 4, True)])
def test_prenorm_forward_backward_parity(golden_dir, monkeypatch, layout, cfg_name, n, ragged):
    """test_forward_backward_parity for pre-norm stacks: golden AudioSet masks, the same clips; loss, activations and parameter
    gradients against the pre-norm oracle in the yardstick forms."""
    cfg = {"small": SMALL, "base": BASE}[cfg_name]
    patch_oracle(monkeypatch, layout)
    m, P = build_pre(cfg, layout)
    m._ensure_engine().ragged = ragged
    ctx, tgt, vis = masks(golden_dir, n)
    audio = clips(n)
    out = m(audio, ctx, tgt, vis)
    assert m._engine.ragged_step == ragged
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(cfg))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(cfg))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    assert out["preds"].shape == ref["preds"].shape and out["preds"].dtype == torch.bfloat16
    if ragged:
        assert float(out["preds"][~seen].float().abs().max()) == 0.0
    tag = f"{layout} {cfg_name} n={n} {'ragged' if ragged else 'dense'}"
    assert_activation_yardstick(out, ref, ref32, seen, tag)
    lo, lr_, l32 = float(out["loss"]), float(ref["loss"]), float(ref32["loss"])
    print(tag, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    assert abs(lo - l32) < 2e-2 * abs(l32), (lo, l32)
    out["loss"].backward()
    ref["loss"].backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gbf = {k: P[k].grad for k in names}
    assert set(names) <= set(got)
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(cfg))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(tag, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()})
    Y.assert_grad_yardstick(table)


@pytest.mark.parametrize("top_k", [8, 1])
def test_prenorm_targets_instance_norm_and_last_layer_paths(golden_dir, monkeypatch, top_k):
    """top_k = 8 (more than the two layers: both kept, instance-normalised over the stream s with the per-clip sums the LayerNorm
    kernel took) and top_k = 1 (the plain last-layer output, no instance norm)."""
    cfg = dict(SMALL, top_k=top_k)
    patch_oracle(monkeypatch)
    m, P = build_pre(cfg)
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    with torch.no_grad():
        out = m(audio, ctx, tgt, vis)
        ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(cfg))
        ref32 = J.jepa_forward(P, audio.float(), *dm, mode="fp32", **oracle_kw(cfg))
    seen = tgt.reshape(-1, vis.shape[-1]).to(dev())
    assert_activation_yardstick(out, ref, ref32, seen, f"top_k={top_k}")
    lo, lr_ = float(out["loss"]), float(ref["loss"])
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)


def test_prenorm_inference_representation(monkeypatch):
    """get_audio_representation on 3 clips, with a key-padding mask on one of them and with None, against J.audio_representation."""
    patch_oracle(monkeypatch)
    m, P = build_pre(SMALL)
    audio = torch.from_numpy(synth.synth_audio(3, 1, 32159, seed=9)).to(dev())
    pad = torch.zeros(3, 200, dtype=torch.bool)
    pad[1, 150:] = True
    kw = dict(spec=SMALL["conv_spec"], enc_heads=SMALL["h_enc"])
    for mask in (pad.to(dev()), None):
        rep = m.get_audio_representation(audio, mask)
        ref = J.audio_representation(P, audio.to(torch.bfloat16), mask, mode="bf16", **kw)
        ref32 = J.audio_representation(P, audio.to(torch.bfloat16).float(), mask, mode="fp32", **kw)
        assert rep.shape == (3, 200, 128) and rep.dtype == torch.float32
        valid = ~pad.to(dev()) if mask is not None else torch.ones(3, 200, dtype=torch.bool, device=dev())
        d_hip, d_orc, pair = rel(rep[valid], ref32[valid]), rel(ref[valid], ref32[valid]), rel(rep[valid], ref[valid])
        print("inference, mask" if mask is not None else "inference, no mask", d_hip, d_orc, pair)
        assert d_hip < Y.ACT_FACTOR * d_orc + Y.ACT_EPS, (d_hip, d_orc)
        assert pair < Y.PAIR_FACTOR * d_orc + Y.ACT_EPS, (pair, d_orc)


@pytest.mark.selfcheck
def test_prenorm_ragged_equals_dense_step(golden_dir):
    """One small 4-clip step in both executions: the same loss (1e-6 relative) and gradients within the bound of
    test_ragged_equals_dense_step (1e-2 relative L2 over all parameters)."""
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4, seed=9)
    res = {}
    for ragged in (True, False):
        m, _ = build_pre(SMALL)
        m._ensure_engine().ragged = ragged
        out = m(audio, ctx, tgt, vis)
        out["loss"].backward()
        assert m._engine.ragged_step == ragged
        res[ragged] = (float(out["loss"]), {k: p.grad.double().clone() for k, p in m.named_parameters() if p.grad is not None})
    (l1, g1), (l0, g0) = res[True], res[False]
    num = sum(float((g1[k] - g0[k]).pow(2).sum()) for k in g0)
    den = sum(float(g0[k].pow(2).sum()) for k in g0)
    print("pre-norm ragged vs dense: loss", l1, l0, "rel", abs(l1 - l0) / abs(l0), "grad rel", (num / den) ** 0.5)
    assert abs(l1 - l0) < 1e-6 * abs(l0), (l1, l0)
    assert (num / den) ** 0.5 < 1e-2, (num / den) ** 0.5


def _runner_steps(m, batches, deterministic):
    """`len(batches)` optimisation steps in StepRunner's order on ready crops (its own crop step draws random offsets)."""
    from wavjepa_amd.trainer import StepRunner
    m.trainer.max_steps = 20
    run = StepRunner(m)
    m._engine.deterministic = deterministic
    losses = []
    for i, batch in enumerate(batches):
        out = m.training_step(batch, i)
        out["loss"].backward()
        run.reducer.wait()
        run.optimizer.step()
        run.scheduler.step()
        m.global_step = i + 1
        losses.append(out["loss"].detach().float().reshape(1).clone())
    m._engine.wait_optimizer()
    torch.cuda.synchronize()
    return run, torch.cat(losses)


def test_prenorm_deterministic_mode(golden_dir, monkeypatch):
    """Two fresh models, three steps each, 4 clips, pinned masks: parameters, Adam moments and losses bit for bit.  And the
    deterministic gradient of one step passes the yardstick the default mode's gradient passes."""
    ctx, tgt, vis = masks(golden_dir, 4)
    batches = [(clips(4, seed=700 + i), ctx, tgt, vis) for i in range(3)]
    runs = []
    for _ in range(2):
        m, _ = build_pre(SMALL, warmup_steps=2)
        _, losses = _runner_steps(m, batches, deterministic=True)
        runs.append((m._flat.p32.clone(), m._flat.t32.clone(), m._flat.adam_m.clone(), m._flat.adam_v.clone(), losses))
    for name, a, b in zip(("parameters", "teacher", "adam_m", "adam_v", "losses"), runs[0], runs[1]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    patch_oracle(monkeypatch)
    audio, dm = batches[0][0], [t.to(dev()) for t in (ctx, tgt, vis)]
    tables = {}
    for det in (True, False):
        m, P = build_pre(SMALL)
        m._ensure_engine().deterministic = det
        out = m(audio, ctx, tgt, vis)
        out["loss"].backward()
        got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        if det:
            names = J.trainable_names(P)
            for k in names:
                P[k].requires_grad_(True)
            J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(SMALL))["loss"].backward()
            gbf = {k: P[k].grad for k in names}
            _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(SMALL))
        tables[det] = Y.grad_yardstick(got, gbf, g32, names, group_of)
        Y.assert_grad_yardstick(tables[det])
    print("deterministic / default grad yardstick ratios:", {g: (round(tables[True][g]["ratio"], 4), round(tables[False][g]["ratio"], 4))
                                                             for g in tables[True]})


def test_prenorm_training_trajectory_vs_oracle(golden_dir, monkeypatch):
    """12 optimisation steps (StepRunner's optimiser, scheduler and order; clip 5) against J.train_step under the monkeypatch, with
    the bounds of test_training_trajectory_vs_oracle -- the existing small-model trajectory test (10 steps there): every loss within
    2e-3 relative, gradient norms within 3e-2, final parameters within 2e-3 relative L2."""
    patch_oracle(monkeypatch)
    m, P = build_pre(SMALL, warmup_steps=3)
    P = {k: v.detach().clone() for k, v in P.items()}
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    from wavjepa_amd.trainer import StepRunner
    m.trainer.max_steps = 20
    run = StepRunner(m)
    ctx, tgt, vis = masks(golden_dir, 6)
    state, worst = {}, 0.0
    for i in range(12):
        sl = slice(2 * (i % 3), 2 * (i % 3) + 2)
        audio = clips(2, seed=100 + i % 3)
        m.global_step = i
        out = m.training_step((audio, ctx[sl], tgt[sl], vis[sl]), i)
        out["loss"].backward()
        run.reducer.wait()
        run.optimizer.step()
        run.scheduler.step()
        r = J.train_step(P, state, i, (audio, ctx[sl].to(dev()), tgt[sl].to(dev()), vis[sl].to(dev())), mode="bf16", warmup=3,
                         total_steps=20, ema=(0.9, 0.99, 10), **oracle_kw(SMALL))
        lo = float(out["loss"])
        worst = max(worst, abs(lo - r["loss"]) / abs(r["loss"]))
        gn = float(run.optimizer.grad_norm())
        assert abs(gn - r["grad_norm"]) < 3e-2 * r["grad_norm"], (i, gn, r["grad_norm"])
    print("pre-norm: worst relative loss deviation over 12 steps:", worst)
    assert worst < 2e-3
    sd = m.state_dict()
    for k in ("encoder.layers.1.linear1.weight", "teacher_encoder.layers.1.linear1.weight", "extract_audio.cnn.2.0.weight",
              "decoder.layers.0.norm1.weight", "decoder.norm.bias"):
        assert rel(sd[k], P[k]) < 2e-3, (k, rel(sd[k], P[k]))


def test_prenorm_launcher_writes_a_checkpoint_the_hear_runtime_loads(tmp_path):
    """`train.py trainer.size=tiny trainer.norm_first=true trainer.steps=3` on the synthetic source in a child process; the
    checkpoint's hyper-parameters carry the flag; RuntimeJEPA(..., norm_first=True) embeds with its weights."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.norm_first=true", "trainer.size=tiny", "trainer.batch_size=1",
           "data.samples_per_audio=4", "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    rc, out, err = launch.run(cmd, cwd=root, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3
    assert ck["hyper_parameters"].get("norm_first_encoder") is True and ck["hyper_parameters"].get("norm_first_decoder") is True
    assert all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    from hear_api.runtime import RuntimeJEPA
    from wavjepa_amd.extractors import ConvFeatureExtractor
    ext = ConvFeatureExtractor(conv_layers_spec=list(J.WAVJEPA_CONV_SPEC), in_channels=1)
    rt = RuntimeJEPA(in_channels=1, weights=ck, is_spectrogram=False, process_seconds=2.01, extractor=ext, model_size="tiny", sr=16000,
                     norm_first=True)
    assert rt.model.encoder.norm_first
    for k in ("encoder.layers.0.linear1.weight", "encoder.norm.weight"):
        assert torch.equal(rt.model.state_dict()[k].cpu(), ck["state_dict"][k])
    wave = torch.from_numpy(synth.synth_audio(2, 1, 50000, seed=31)).float()[:, 0]
    emb, ts = rt.get_timestamp_embeddings(wave)
    assert emb.shape[0] == 2 and emb.shape[2] == rt.timestamp_embedding_size == 128 and emb.shape[1] == ts.shape[1]
    assert bool(torch.isfinite(emb).all())
    scene = rt.get_scene_embeddings(wave)
    assert scene.shape == (2, 128) and bool(torch.isfinite(scene).all())


def test_post_norm_step_reaches_none_of_the_pre_norm_code(golden_dir, monkeypatch):
    """The default layout: one small step (forward, teacher, backward, inference) never calls the new entries; a pre-norm model
    calls no post-norm LayerNorm between the front-end's and the conv stack's."""
    from wavjepa_amd import ops
    calls = {}

    def counted(name):
        fn = getattr(ops, name)

        def wrapper(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)
    for name in ("layernorm_pre_fwd", "layernorm_pre_bwd", "ln_pre_bwd_partial_rows", "layernorm_fwd", "layernorm_bwd"):
        counted(name)
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4)
    m, _ = build(SMALL)
    out = m(audio, ctx, tgt, vis)
    out["loss"].backward()
    m.get_audio_representation(audio.float(), None)
    torch.cuda.synchronize()
    assert not any(k in calls for k in ("layernorm_pre_fwd", "layernorm_pre_bwd", "ln_pre_bwd_partial_rows")), calls
    post = dict(calls)
    calls.clear()
    m, _ = build_pre(SMALL)
    out = m(audio, ctx, tgt, vis)
    out["loss"].backward()
    m.get_audio_representation(audio.float(), None)
    torch.cuda.synchronize()
    # feature_norms only: one forward per front-end pass (training step + inference), one backward
    assert calls.get("layernorm_fwd") == 2 and calls.get("layernorm_bwd") == 1, calls
    # per stack 2 norms per layer + the final norm; the teacher one more (its last residual add); inference the student again
    assert calls.get("layernorm_pre_fwd") == 3 * (2 * 2 + 1) + (2 * 2 + 1), calls
    assert calls.get("layernorm_pre_bwd") == 2 * (2 * 2 + 1), calls
    assert post.get("layernorm_fwd", 0) > 2 and post.get("layernorm_bwd", 0) > 1
