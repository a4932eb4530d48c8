"""Clips of more than 416 tokens through the HIP engine (the block-streamed attention entries) against the oracle (GPU only).

The small model of tests/test_jepa_gpu.py (64-wide student heads, 32-wide predictor heads) behind the seven-layer conv geometry of the
full model at width 64 (stride 320, so that seconds and tokens are the workload's) at 8.41 s = 420 tokens -- the smallest
convenient length above the whole-image kernels' limit -- and at 10 s = 499 tokens, the corpus' clip length.  Bounds: the yardstick
forms of tests/parity_yardstick.py (d(HIP, fp32) against d(oracle-bf16, fp32) on the same draw: factor 1.1 / eps 2e-4 for activations,
1.25 / 5e-4 for gradient groups) and the loss within 1e-3 relative of the oracle's bf16 flow.  Masks: the oracle's AudioSet masker
under a seeded generator, as tests/test_jepa_gpu.py::masks draws them.  Every test prints its distances before it asserts."""
import gc

import numpy as np
import pytest
import torch

import synth
from oracle import jepa_oracle as J
from oracle import masking_oracle as MO
from tests import parity_yardstick as Y
from tests.test_jepa_gpu import SMALL, SMALL_SPEC, build, dev, group_of, oracle_kw, rel
from tests.test_prenorm_gpu import assert_activation_yardstick, build_pre, patch_oracle

pytestmark = pytest.mark.gpu

CFG = dict(SMALL, conv_spec=SMALL_SPEC + [(64, 2, 2)])      # (10,5) (3,2)x4 (2,2)x2: 320 samples per token, 160 000 samples -> 499 tokens
LENGTHS = {420: (8.41, 134560), 499: (10.0, 160000), 999: (10.0, 160000)}       # tokens: (seconds, samples)
CFG_OF = {420: CFG, 499: CFG, 999: SMALL}                   # 999: the same 10 s behind the six-layer stack (stride 160) of the default extractor


def drawn_masks(n, T, seed=1234):
    rng = np.random.default_rng(seed)
    return tuple(torch.from_numpy(a) for a in MO.time_inverse_block_masks(
        n, T, 1, new_rng=lambda: np.random.default_rng(rng.integers(1 << 31))))


def long_model(T, builder=build, **kw):
    seconds, samples = LENGTHS[T]
    m, P = builder(CFG_OF[T], seconds=seconds, tokens=T, **kw)
    assert m.total_patches == T and m.target_length == samples
    return m, P


def clips(n, T, seed=3):
    return torch.from_numpy(synth.synth_audio(n, 1, LENGTHS[T][1], seed=seed)).to(torch.bfloat16).to(dev())


def recorded_attention_calls(monkeypatch):
    """every attention launch of the engine as (entry, T of the call)"""
    from wavjepa_amd import ops
    calls = []
    for name in ("attn_fwd", "attn_bwd", "attn_stream_fwd", "attn_stream_bwd"):
        real = getattr(ops, name)

        def wrapped(*a, _real=real, _name=name, **kw):
            calls.append((_name, kw["T"]))
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, wrapped)
    return calls


def step_parity(m, P, T, n, ragged, tag):
    CFG = CFG_OF[T]
    m._ensure_engine().ragged = ragged
    ctx, tgt, vis = drawn_masks(n, T)
    audio = clips(n, T)
    out = m(audio, ctx, tgt, vis)
    assert m._engine.ragged_step == ragged
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(CFG))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(CFG))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    assert out["preds"].shape == ref["preds"].shape
    lo, lr_, l32 = float(out["loss"]), float(ref["loss"]), float(ref32["loss"])
    print(tag, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32, "rel", abs(lo - lr_) / abs(lr_), flush=True)
    assert_activation_yardstick(out, ref, ref32, seen, tag)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    out["loss"].backward()
    ref["loss"].backward()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gbf = {k: P[k].grad for k in names}
    assert set(names) <= set(got)
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(CFG))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(tag, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()}, flush=True)
    Y.assert_grad_yardstick(table)


@pytest.mark.parametrize("T,ragged", [(420, False), (420, True), (499, False), (499, True), (999, True)])
def test_forward_backward_parity_beyond_416_tokens(monkeypatch, T, ragged):
    """dense: all three stacks run the streamed kernels at the full T under key masks and mask_group; ragged: the teacher does, the
    student and the predictor by the length of their longest visible set."""
    calls = recorded_attention_calls(monkeypatch)
    m, P = long_model(T)
    step_parity(m, P, T, 2, ragged, f"{T} tokens {'ragged' if ragged else 'dense'}")
    print("attention launches:", sorted(set(calls)), flush=True)
    for name, t in calls:
        assert ("stream" in name) == (t > 416), (name, t)
    assert ("attn_stream_fwd", T) in calls                       # the teacher, always at the full length
    if not ragged:
        assert {c for c in calls} == {("attn_stream_fwd", T), ("attn_stream_bwd", T)}


def test_inference_representation_at_499_tokens():
    m, P = long_model(499)
    audio = torch.from_numpy(synth.synth_audio(2, 1, 160000, seed=9)).to(dev())
    pad = torch.zeros(2, 499, dtype=torch.bool)
    pad[:, 499 - 130:] = True
    kw = dict(spec=CFG["conv_spec"], enc_heads=CFG["h_enc"])
    for mask in (None, pad.to(dev())):
        rep = m.get_audio_representation(audio, mask)
        ref = J.audio_representation(P, audio.to(torch.bfloat16), mask, mode="bf16", **kw)
        ref32 = J.audio_representation(P, audio.to(torch.bfloat16).float(), mask, mode="fp32", **kw)
        valid = slice(0, 499 - 130) if mask is not None else slice(0, 499)
        pair, d_hip, d_orc = rel(rep[:, valid], ref[:, valid]), rel(rep[:, valid], ref32[:, valid]), rel(ref[:, valid], ref32[:, valid])
        print("inference at 499 tokens,", "padding mask" if mask is not None else "no mask", "pair / d_hip / d_orc:", pair, d_hip, d_orc, flush=True)
        assert rep.shape == (2, 499, 128) and rep.dtype == torch.float32
        assert pair < 1e-2                                        # the bound of tests/test_jepa_gpu.py::test_inference_representation
        assert d_hip < Y.ACT_FACTOR * d_orc + Y.ACT_EPS, (d_hip, d_orc)


def test_prenorm_dense_step_at_420_tokens(monkeypatch):
    patch_oracle(monkeypatch)
    m, P = long_model(420, builder=build_pre)
    step_parity(m, P, 420, 2, False, "pre-norm 420 tokens dense")


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16).clone()


def _fresh_step(T, deterministic, n=2, seed=3):
    """a freshly built model's first forward + backward: (loss bits, gradient buffer bits)"""
    if T in LENGTHS:
        m, _ = long_model(T)
    else:
        m, _ = build(SMALL)
    eng = m._ensure_engine()
    eng.deterministic = deterministic
    ctx, tgt, vis = drawn_masks(n, T, seed=77)
    samples = LENGTHS[T][1] if T in LENGTHS else 32159
    audio = torch.from_numpy(synth.synth_audio(n, 1, samples, seed=seed)).to(torch.bfloat16).to(dev())
    out = m(audio, ctx, tgt, vis)
    out["loss"].backward()
    torch.cuda.synchronize()
    res = _bits(out["loss"].float().reshape(1)), _bits(m._flat.g32)
    assert bool(torch.isfinite(m._flat.g32).all())
    del m, out
    gc.collect()
    torch.cuda.empty_cache()
    return res


def test_deterministic_step_at_420_tokens_is_bit_identical():
    a, b = _fresh_step(420, True), _fresh_step(420, True)
    print("deterministic 420-token step: loss bits equal", bool(torch.equal(a[0], b[0])), "differing gradient words",
          int((a[1] != b[1]).sum()), flush=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_short_clips_are_untouched_by_a_long_model_in_the_process():
    """200 tokens take the whole-image kernels, before and after a 499-token model ran (deterministic mode, so that equal means
    bit-identical)."""
    before = _fresh_step(200, True)
    _fresh_step(499, True)
    after = _fresh_step(200, True)
    print("200-token step around a 499-token one: differing gradient words", int((before[1] != after[1]).sum()), flush=True)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_three_optimiser_steps_at_420_tokens_follow_the_oracle():
    """the loop and the bounds of tests/test_jepa_gpu.py::test_training_trajectory_vs_oracle, three steps at 420 tokens"""
    m, P = long_model(420, warmup_steps=3)
    P = {k: v.detach().clone() for k, v in P.items()}
    m.trainer.max_steps = 20
    m.hparams["ema_decay"], m.hparams["ema_end_decay"], m.ema_end_step = 0.9, 0.99, 10
    oc = m.configure_optimizers()
    opt, sch = oc["optimizer"], oc["lr_scheduler"]["scheduler"]
    opt.max_grad_norm = 5.0
    ctx, tgt, vis = drawn_masks(6, 420)
    state, worst = {}, 0.0
    for i in range(3):
        sl = slice(2 * i, 2 * i + 2)
        audio = clips(2, 420, seed=100 + i)
        m.global_step = i
        out = m.training_step((audio, ctx[sl], tgt[sl], vis[sl]), i)
        out["loss"].backward()
        opt.step()
        sch.step()
        r = J.train_step(P, state, i, (audio, ctx[sl].to(dev()), tgt[sl].to(dev()), vis[sl].to(dev())), mode="bf16", warmup=3,
                         total_steps=20, ema=(0.9, 0.99, 10), **oracle_kw(CFG))
        lo, gn = float(out["loss"]), float(opt.grad_norm())
        print(f"step {i}: loss hip / oracle {lo} / {r['loss']}, grad norm {gn} / {r['grad_norm']}", flush=True)
        assert np.isfinite(lo)
        worst = max(worst, abs(lo - r["loss"]) / abs(r["loss"]))
        assert abs(gn - r["grad_norm"]) < 3e-2 * r["grad_norm"], (i, gn, r["grad_norm"])
    print("worst relative loss deviation over 3 steps at 420 tokens:", worst, flush=True)
    assert worst < 2e-3


def test_tiny_heads_beyond_416_tokens_are_refused_at_construction():
    """16-wide heads have no streamed kernel: a clear error when the engine is built, not a -3 inside a step"""
    m, _ = long_model(420)
    m.n_decoder_heads = 4                       # 64 / 4 = 16-wide predictor heads
    m._engine = None
    with pytest.raises(NotImplementedError, match="16-wide decoder heads"):
        m._ensure_engine()


def test_denoiser_step_on_ten_second_clips():
    """Denoiser(process_audio_seconds=10.0): dense 2N clips of 499 tokens, no mask, through the streamed kernels, at the bounds of
    tests/test_denoiser_gpu.py::test_denoiser_forward_backward_parity_vs_oracle (losses 1e-3, gradient groups 3e-2)."""
    from oracle import denoiser_oracle as DN
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    spec, d = CFG["conv_spec"], 128
    den = Denoiser(ConvFeatureExtractor(conv_layers_spec=spec, in_channels=1), TransformerLayerCFG.create(d_model=d, nhead=2),
                   TransformerEncoderCFG.create(num_layers=2), alpha=0.3, lr=1e-3, nr_samples_per_audio=2, process_audio_seconds=10.0)
    tea = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=spec, in_channels=1),
               transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=2),
               transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=d, nhead=2),
               transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=2),
               transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2), average_top_k_layers=2,
               process_audio_seconds=10.0, nr_samples_per_audio=2)
    P, PT = {}, {}
    for mod, store, sd_seed in ((den, P, 11), (tea, PT, 12)):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed=sd_seed).items() if k in shapes}
        sd["pos_encoding_encoder"] = J.sincos_positions(d, 499)
        if "pos_encoding_decoder" in shapes:
            sd["pos_encoding_decoder"] = J.sincos_positions(64, 499)
        mod.load_state_dict(sd)
        store.update({k: v.clone().to(dev()) for k, v in sd.items()})
    den = den.to(dev())
    den._set_teacher(tea.to(dev()))
    clean = torch.from_numpy(synth.synth_audio(2, 1, 160000, seed=41)).to(torch.bfloat16).to(dev())
    noise = torch.from_numpy(synth.synth_audio(2, 1, 160000, seed=42)).to(dev())
    generated = (clean.float() + 0.5 * noise).to(torch.bfloat16)
    out = den(generated, clean)
    names = [k for k in P if k != "pos_encoding_encoder"]
    for k in names:
        P[k].requires_grad_(True)
    ref = DN.denoiser_forward(P, PT, generated, clean, alpha=0.3, spec=spec, enc_heads=2, mode="bf16")
    losses = {k: (float(out[k].detach()), float(ref[k].detach())) for k in ("loss", "loss_clean", "loss_denoise_dereverb")}
    out["loss"].backward()
    ref["loss"].backward()
    got = {k: p.grad for k, p in den.named_parameters() if p.grad is not None}
    errs = Y.group_errors(got, {k: P[k].grad for k in names}, names, group_of)
    print("denoiser at 499 tokens: losses (hip, oracle)", losses, "grad rel errors per group:", errs, flush=True)
    for k, (a, b) in losses.items():
        assert abs(a - b) < 1e-3 * abs(b), (k, a, b)
    for g, e in errs.items():
        assert e < 3e-2, (g, e)


def test_hear_runtime_embeds_with_ten_second_windows():
    """hear_api.RuntimeJEPA(process_seconds=10): one clip of 10.6 s = two windows of 499 tokens, the second mostly padding (a key
    mask over its tail), against the oracle's restatement at the bound of tests/test_jepa_gpu.py's HEAR test (2e-2)."""
    from hear_api.runtime import RuntimeJEPA
    from oracle import hear_oracle as HO
    from wavjepa_amd.extractors import ConvFeatureExtractor
    spec = list(J.WAVJEPA_CONV_SPEC) + [(512, 2, 2)]             # configs/extractor/wav2vec2.yaml: stride 320, 10 s -> 499 tokens
    ext = ConvFeatureExtractor(conv_layers_spec=spec, in_channels=1)
    rt = RuntimeJEPA(in_channels=1, weights=None, is_spectrogram=False, process_seconds=10, extractor=ext, model_size="base", sr=16000)
    assert rt.model.total_patches == 499
    shapes = {k: tuple(v.shape) for k, v in rt.model.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in synth.synth_state_dict(shapes, seed=23).items()}
    sd["pos_encoding_encoder"] = J.sincos_positions(768, 499)
    sd["pos_encoding_decoder"] = J.sincos_positions(384, 499)
    rt.model.load_state_dict(sd)
    wave = torch.from_numpy(synth.synth_audio(1, 1, 170000, seed=31)).float()[:, 0]
    emb, ts = rt.get_timestamp_embeddings(wave)
    ref, ref_ts = HO.timestamp_embeddings(sd, rt.to_feature(wave).cpu(), process_seconds=10, spec=spec, mode="fp32")
    print("hear runtime, 10 s windows:", tuple(emb.shape), "rel", rel(emb, ref), flush=True)
    assert emb.shape == ref.shape and ts.shape == ref_ts.shape
    assert torch.allclose(ts.cpu(), ref_ts, atol=1e-3)
    assert rel(emb, ref) < 2e-2, rel(emb, ref)
