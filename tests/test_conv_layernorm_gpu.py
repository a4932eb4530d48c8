"""End-to-end parity of the mode="layer_norm" conv front-end (Conv1d(+bias) -> LayerNorm over channels -> GELU in every layer)
through the HIP engine against the oracle (GPU only).

The oracle becomes the oracle of this mode by replacing its conv stack (tests/conv_layernorm_reference.py, pinned to the reference's
extractor classes by tests/test_conv_layernorm_cpu.py).  Masks, clips, yardstick assertions and loss bounds are those of
tests/test_prenorm_gpu.py: loss within 1e-3 of the oracle's bf16 flow and 2e-2 of its fp32 flow, activations and parameter-gradient
groups in the yardstick forms of tests/parity_yardstick.py.
"""
import functools

import numpy as np
import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import parity_yardstick as Y
from tests.conv_layernorm_reference import conv_stack_layer_norm
from tests.test_jepa_gpu import BASE, SMALL, PinnedRng, build, channel_group_of, dev, group_of, masks, oracle_kw, rel
from tests.test_prenorm_gpu import assert_activation_yardstick, build_pre, clips
from tests.test_prenorm_gpu import patch_oracle as patch_prenorm

pytestmark = pytest.mark.gpu


def build_ln(cfg, conv_bias=True, builder=build, **kw):
    """tests.test_jepa_gpu.build (or build_pre) with both extractor classes constructed in mode="layer_norm"; LayerNorm gains around 1
    (synth's rule for names under `cnn.` draws conv weights)."""
    import wavjepa_amd.extractors as E
    saved = E.ConvFeatureExtractor, E.ConvChannelFeatureExtractor
    E.ConvFeatureExtractor = functools.partial(saved[0], mode="layer_norm", conv_bias=conv_bias)
    E.ConvChannelFeatureExtractor = functools.partial(saved[1], mode="layer_norm", conv_bias=conv_bias)
    try:
        m, P = builder(cfg, **kw)
    finally:
        E.ConvFeatureExtractor, E.ConvChannelFeatureExtractor = saved
    assert m.extract_audio.mode == "layer_norm" and m.extract_audio.conv_bias == conv_bias
    gains = {k: torch.from_numpy((1.0 + 0.1 * synth.hash_uniform(v.numel(), synth.name_seed(k, 7))).astype(np.float32)).to(dev())
             for k, v in P.items() if k.endswith(".2.1.weight")}
    assert len(gains) == len(cfg["conv_spec"]) * max(1, len(getattr(m.extract_audio, "cnns", [0])))
    m.load_state_dict(gains, strict=False)
    P.update({k: v.clone() for k, v in gains.items()})
    return m, P


def patch_oracle(monkeypatch):
    monkeypatch.setattr(J, "_conv_stack", conv_stack_layer_norm)


def step_parity(m, P, cfg, audio, ctx, tgt, vis, ragged, tag, groups=group_of):
    """One step of m against the patched oracle: loss bounds, activation yardstick, gradient yardstick per group."""
    m._ensure_engine().ragged = ragged
    out = m(audio, ctx, tgt, vis)
    assert m._engine.ragged_step == ragged and m._engine.conv_ln
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(cfg))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(cfg))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    assert out["preds"].shape == ref["preds"].shape
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
    table = Y.grad_yardstick(got, gbf, g32, names, groups)
    print(tag, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()})
    Y.assert_grad_yardstick(table)
    return table


@pytest.mark.parametrize("cfg_name,n,ragged,conv_bias", [("small", 4, True, True), ("small", 4, True, False), ("small", 4, False, True),
                                                         ("small", 4, False, False), ("small", 1, True, True), ("base", 2, True, True)])
def test_conv_layernorm_forward_backward_parity(golden_dir, monkeypatch, cfg_name, n, ragged, conv_bias):
    cfg = {"small": SMALL, "base": BASE}[cfg_name]
    patch_oracle(monkeypatch)
    m, P = build_ln(cfg, conv_bias)
    assert ("extract_audio.cnn.3.0.bias" in P) == conv_bias and "extract_audio.cnn.0.2.weight" not in P
    ctx, tgt, vis = masks(golden_dir, n)
    step_parity(m, P, cfg, clips(n), ctx, tgt, vis, ragged, f"layer_norm {cfg_name} n={n} {'ragged' if ragged else 'dense'} bias={conv_bias}")


def test_conv_layernorm_with_pre_norm_stacks(golden_dir, monkeypatch):
    patch_oracle(monkeypatch)
    patch_prenorm(monkeypatch)
    m, P = build_ln(SMALL, True, builder=build_pre)
    assert m.encoder.norm_first and m.decoder.norm_first
    ctx, tgt, vis = masks(golden_dir, 4)
    step_parity(m, P, SMALL, clips(4), ctx, tgt, vis, True, "layer_norm + norm_first small n=4 ragged")


@pytest.mark.parametrize("stacks", ["own", "shared"])
def test_conv_layernorm_channel_extractor(monkeypatch, stacks):
    """ConvChannelFeatureExtractor: 3 two-channel clips, every channel through its own (or the shared) mono stack; each stack's
    gradient group on its own (channel_group_of, with parity_yardstick's factor for `extract_audio.cnns`)."""
    from wavjepa_amd.masking import TimeInverseBlockMasker
    patch_oracle(monkeypatch)
    m, P = build_ln(SMALL, True, seconds=1.0, tokens=198, in_channels=2, channel_stacks=stacks)
    with PinnedRng(4100):
        ctx, tgt, vis = TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1, channel_based_masking=True, channel_major=True)(
            batch_size=3, n_times=198, in_channels=2)
    audio = torch.from_numpy(synth.synth_audio(3, 2, 16000, seed=31)).to(torch.bfloat16).to(dev())
    table = step_parity(m, P, SMALL, audio, ctx, tgt, vis, True, f"layer_norm channel stacks {stacks}", groups=channel_group_of)
    assert m._engine.S == 2 and len(m._engine.stacks) == (2 if stacks == "own" else 1)
    assert sum(1 for g in table if g.startswith("extract_audio.cnns")) == (2 if stacks == "own" else 1)
    tok = m.extract_audio(audio)                                     # the stand-alone extractor forward runs the same kernels
    want = J.conv_frontend({k: v.detach() for k, v in P.items()}, audio, SMALL["conv_spec"], "bf16")
    want32 = J.conv_frontend({k: v.detach() for k, v in P.items()}, audio.float(), SMALL["conv_spec"], "fp32")
    d_hip, d_orc = rel(tok.float(), want32), rel(want.float(), want32)
    print("stand-alone tokens: d(HIP, fp32)", d_hip, "d(oracle-bf16, fp32)", d_orc)
    assert tok.shape == want.shape == (3, 198, 64) and tok.dtype == torch.bfloat16
    assert d_hip < Y.ACT_FACTOR * d_orc + Y.ACT_EPS


@pytest.mark.parametrize("channels", [None, "own", "shared"])
@pytest.mark.parametrize("mode", ["default", "layer_norm"])
def test_engine_front_end_and_stand_alone_extractor_give_the_same_tokens(mode, channels):
    """3 clips of 16000 samples, mono (99 tokens) or two channels through own / shared stacks (198 tokens): after an inference pass the
    engine front-end's token slice and the stand-alone m.extract_audio(audio) are the same bits -- both callers run one walker."""
    kw = dict(seconds=1.0, tokens=99) if channels is None else dict(seconds=1.0, tokens=198, in_channels=2, channel_stacks=channels)
    m, _ = build(SMALL, **kw) if mode == "default" else build_ln(SMALL, True, **kw)
    audio = torch.from_numpy(synth.synth_audio(3, 1 if channels is None else 2, 16000, seed=31)).to(torch.bfloat16).to(dev())
    m.get_audio_representation(audio, None)
    got = m._engine.front.tokens()
    want = m.extract_audio(audio)
    assert m._engine.conv_ln == (mode == "layer_norm") and len(m._engine.stacks) == (2 if channels == "own" else 1)
    assert got.shape == want.shape == (3, 99 if channels is None else 198, 64) and got.dtype == want.dtype == torch.bfloat16
    assert float(want.float().abs().max()) > 0 and torch.equal(got, want)


def test_conv_layernorm_inference_representation(monkeypatch):
    """get_audio_representation on 3 clips, with a key-padding mask on one of them and with None, against J.audio_representation."""
    patch_oracle(monkeypatch)
    m, P = build_ln(SMALL, True)
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


def test_conv_layernorm_three_steps_vs_oracle(golden_dir, monkeypatch):
    """Three optimisation steps (clip 5, AdamW with weight decay on every parameter, warm-up) against J.train_step under the patch, with
    the bounds of test_training_trajectory_vs_oracle: every loss within 2e-3 relative, gradient norms within 3e-2; the new parameters
    (conv bias, LayerNorm gain and bias) end within 2e-3 relative L2 of the oracle's."""
    patch_oracle(monkeypatch)
    m, P = build_ln(SMALL, True, warmup_steps=3)
    P = {k: v.detach().clone() for k, v in P.items()}
    m.trainer.max_steps = 20
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    oc = m.configure_optimizers()
    opt, sch = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    opt.max_grad_norm = 5.0
    ctx, tgt, vis = masks(golden_dir, 6)
    state, worst = {}, 0.0
    for i in range(3):
        sl = slice(2 * i, 2 * i + 2)
        audio = clips(2, seed=100 + i)
        m.global_step = i
        out = m.training_step((audio, ctx[sl], tgt[sl], vis[sl]), i)
        out["loss"].backward()
        opt.step()
        sch.step()
        r = J.train_step(P, state, i, (audio, ctx[sl].to(dev()), tgt[sl].to(dev()), vis[sl].to(dev())), mode="bf16", warmup=3,
                         total_steps=20, ema=(0.9, 0.99, 10), **oracle_kw(SMALL))
        lo = float(out["loss"])
        worst = max(worst, abs(lo - r["loss"]) / abs(r["loss"]))
        gn = float(opt.grad_norm())
        assert abs(gn - r["grad_norm"]) < 3e-2 * r["grad_norm"], (i, gn, r["grad_norm"])
    print("layer_norm: worst relative loss deviation over 3 steps:", worst)
    assert worst < 2e-3
    sd = m.state_dict()
    for k in ("extract_audio.cnn.2.0.weight", "extract_audio.cnn.2.0.bias", "extract_audio.cnn.0.2.1.weight", "extract_audio.cnn.5.2.1.bias",
              "encoder.layers.1.linear1.weight"):
        assert rel(sd[k], P[k]) < 2e-3, (k, rel(sd[k], P[k]))
    lo_, hi_ = m._flat.by_name["extract_audio.cnn.5.2.1.bias"].offset, m._flat.n
    assert 0 <= lo_ < hi_ and any(lo <= lo_ < hi for lo, hi in m._flat.front_and_rest_ranges()[0])     # in the front gradient section
    assert any(lo <= lo_ < hi for lo, hi in m._flat.bucket_bounds(4))


def one_step_g32(m, audio, ctx, tgt, vis, deterministic=True):
    m._ensure_engine().deterministic = deterministic
    out = m(audio, ctx, tgt, vis)
    out["loss"].backward()
    torch.cuda.synchronize()
    return m._flat.g32.clone().view(torch.int32), out["loss"].detach().float().reshape(1).clone().view(torch.int32)


@pytest.mark.parametrize("ragged", [True, False])
def test_conv_layernorm_deterministic_mode(golden_dir, ragged):
    """The same step twice on fresh models gives equal g32 bits (ragged: listed-rows kernels, dense: dense forms)."""
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4, seed=700)
    res = []
    for _ in range(2):
        m, _ = build_ln(SMALL, True)
        m._ensure_engine().ragged = ragged
        res.append(one_step_g32(m, audio, ctx, tgt, vis))
        assert m._engine.ragged_step == ragged
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0], res[1][0])
    assert bool(torch.isfinite(res[0][0].view(torch.float32)).all())


def test_default_mode_is_untouched_by_a_layer_norm_model_in_the_process(golden_dir, monkeypatch):
    """mode="default": g32 of one SMALL step in deterministic mode, before and after a layer_norm model was built and stepped in the same
    process, bit for bit -- and the default step calls none of the new entries."""
    from wavjepa_amd import ops
    ctx, tgt, vis = masks(golden_dir, 4)
    audio = clips(4, seed=700)
    calls = {}
    for name in ("conv_ln_gelu_fwd", "conv_ln_gelu_bwd", "conv0_ln_fwd", "conv0_ln_bwd", "conv_ln_bwd_partial_rows"):
        fn = getattr(ops, name)

        def wrapper(*a, _fn=fn, _name=name, **k):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a, **k)
        monkeypatch.setattr(ops, name, wrapper)
    m, _ = build(SMALL)
    before = one_step_g32(m, audio, ctx, tgt, vis)
    assert not calls, calls
    ln, _ = build_ln(SMALL, True)
    one_step_g32(ln, audio, ctx, tgt, vis)
    ln.get_audio_representation(audio.float(), None)
    assert calls.get("conv0_ln_fwd") == 2 and calls.get("conv0_ln_bwd") == 1 and calls.get("conv_ln_gelu_fwd") == 10 and calls.get("conv_ln_gelu_bwd") == 5
    calls.clear()
    m2, _ = build(SMALL)
    after = one_step_g32(m2, audio, ctx, tgt, vis)
    again = one_step_g32(m, audio, ctx, tgt, vis)                    # the first model, stepped again
    assert not calls, calls
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and torch.equal(before[0], again[0])


def test_conv_layernorm_refusals_at_engine_construction():
    m, _ = build_ln(SMALL, True)
    eng = m._ensure_engine()
    eng.fp8 = True
    with pytest.raises(RuntimeError, match="layer_norm"):
        eng._check_fp8()
    eng.fp8 = False


def test_conv_layernorm_checkpoint_resume_is_bit_exact(tmp_path):
    """2 steps, save, a fresh start that loads the checkpoint, 1 more step, against 3 uninterrupted steps on identical batches in
    deterministic mode: parameters (conv bias and LayerNorm parameters among them), Adam moments and the teacher are bit-equal at step 3,
    i.e. the step after the resume computed the same loss and gradient bits."""
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
        m, _ = build_ln(SMALL, True, seed=seed, warmup_steps=2)
        tr = Trainer(max_steps=3, default_root_dir=str(root), checkpoint_every_n_steps=1, log_every_n_steps=0, deterministic=True)
        tr.fit(m, train_dataloaders=loader(skip), ckpt_path=ckpt)
        return m

    ma = run(7, tmp_path / "a")
    mb = run(8, tmp_path / "b", ckpt=str(tmp_path / "a" / "step=2.ckpt"), skip=2)
    a = torch.load(tmp_path / "a" / "step=3.ckpt", map_location="cpu", weights_only=False)
    b = torch.load(tmp_path / "b" / "step=3.ckpt", map_location="cpu", weights_only=False)
    assert a["global_step"] == b["global_step"] == 3
    assert "extract_audio.cnn.4.0.bias" in a["state_dict"] and "extract_audio.cnn.4.2.1.weight" in a["state_dict"]
    assert set(a["state_dict"]) == set(b["state_dict"])
    for k, va in a["state_dict"].items():
        assert torch.equal(va, b["state_dict"][k]), k
    for k in ("m", "v"):
        assert torch.equal(a["optimizer"][k], b["optimizer"][k]), k
    torch.cuda.synchronize()
    assert torch.equal(ma._flat.p32, mb._flat.p32) and torch.equal(ma._flat.t32, mb._flat.t32)
