"""Dropout in the student and the predictor through the HIP engine (GPU only).

The DEEP model of tests/test_recompute_gpu.py (7 student layers of width 128 with 2 heads of 64, 5 predictor layers of width 64 with 2
heads of 32), 4 clips of 2.01 s, the golden AudioSet masks, p = 0.1.  The oracle is given the engine's masks, rebuilt on the host bit
for bit (tests/dropout_reference.py), so a dropout step is held to the same yardstick forms and constants as a step without it.
Every test prints its figures before it asserts."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import synth
from oracle import jepa_oracle as J
from tests import dropout_reference as R
from tests import launch
from tests import parity_yardstick as Y
from tests.test_jepa_gpu import dev, group_of, masks, oracle_kw
from tests.test_prenorm_gpu import assert_activation_yardstick
from tests.test_recompute_gpu import DEEP, N_CLIPS, bits, differing

pytestmark = pytest.mark.gpu

P_DROP = 0.1
SEED = 20240607


def build_drop(p_enc, p_dec, seed=7, teacher_scale=0.97, dropout_seed=SEED, **kw):
    """tests/test_jepa_gpu.py::build with the two dropout rates in the layer configs (the same synthetic weights)"""
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    cfg = DEEP
    m = JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=cfg["conv_spec"], in_channels=1),
             transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=cfg["l_enc"]),
             transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=cfg["d_enc"], nhead=cfg["h_enc"], dropout=p_enc),
             transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=cfg["l_dec"]),
             transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=cfg["d_dec"], nhead=cfg["h_dec"], dropout=p_dec),
             lr=4e-4, adam_betas=(0.9, 0.98), adam_weight_decay=0.04, average_top_k_layers=cfg["top_k"],
             process_audio_seconds=2.01, nr_samples_per_audio=2, **kw)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = synth.synth_state_dict(shapes, seed=seed)
    for k in list(sd):
        if k.startswith("teacher_encoder.") and k.endswith("weight") and sd[k].ndim == 2:
            sd[k] = (sd[k] * np.float32(teacher_scale)).astype(np.float32)
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    sd["pos_encoding_encoder"] = J.sincos_positions(cfg["d_enc"], 200)
    sd["pos_encoding_decoder"] = J.sincos_positions(cfg["d_dec"], 200)
    m.load_state_dict(sd)
    m.dropout_seed = dropout_seed
    P = {k: v.clone().to(dev()) for k, v in sd.items()}
    return m.to(dev()), P


def draw(golden_dir, seed=3):
    audio = torch.from_numpy(synth.synth_audio(N_CLIPS, 1, 32159, seed=seed)).to(torch.bfloat16).to(dev())
    return audio, masks(golden_dir, N_CLIPS)


def one_step(golden_dir, p_enc=P_DROP, p_dec=P_DROP, deterministic=True, call=None, attrs=None, **kw):
    m, _ = build_drop(p_enc, p_dec, **kw)
    eng = m._ensure_engine()
    eng.deterministic = deterministic
    for k, v in (attrs or {}).items():
        setattr(eng, k, v)
    m.dropout_call = call
    audio, mset = draw(golden_dir)
    out = m(audio, *mset)
    out["loss"].backward()
    torch.cuda.synchronize()
    return bits(out["loss"].detach().float().reshape(1)), m._flat.g32.clone(), m


# ------------------------------------------------------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("form", ["dense", "ragged"])
def test_dropout_step_against_the_oracle_with_the_same_masks(golden_dir, monkeypatch, form):
    m, P = build_drop(P_DROP, P_DROP)
    eng = m._ensure_engine()
    ragged = form == "ragged"
    eng.ragged = ragged
    m.dropout_call = 5
    audio, (ctx, tgt, vis) = draw(golden_dir)
    assert m.training
    out = m(audio, ctx, tgt, vis)
    assert eng.ragged_step == ragged and eng._drop_now == dict(enc=P_DROP, dec=P_DROP)
    provider = R.EngineMasks(m._dropout_key(), 5, dict(enc=P_DROP, dec=P_DROP), dev(), plan=eng.plan if ragged else None,
                             tail=eng.tail is not None)
    provider.n_layers = dict(enc=DEEP["l_enc"], dec=DEEP["l_dec"])
    R.install(monkeypatch, provider)
    names = J.trainable_names(P)
    for k in names:
        P[k].requires_grad_(True)
    dm = [t.to(dev()) for t in (ctx, tgt, vis)]
    ref = J.jepa_forward(P, audio, *dm, mode="bf16", **oracle_kw(DEEP))
    ref32 = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio.float(), *dm, mode="fp32", **oracle_kw(DEEP))
    seen = (tgt if ragged else ~vis).reshape(-1, vis.shape[-1]).to(dev())
    preds = out["preds"].clone()
    lo, lr_, l32 = float(out["loss"].detach()), float(ref["loss"].detach()), float(ref32["loss"])
    print(form, "loss hip/oracle-bf16/oracle-fp32:", lo, lr_, l32, "rel", abs(lo - lr_) / abs(lr_), flush=True)
    assert_activation_yardstick(out, ref, ref32, seen, "dropout-" + form)
    assert abs(lo - lr_) < 1e-3 * abs(lr_), (lo, lr_)
    assert abs(lo - l32) < 2e-2 * abs(l32), (lo, l32)
    out["loss"].backward()
    ref["loss"].backward()
    torch.cuda.synchronize()
    got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    gbf = {k: P[k].grad for k in names}
    assert set(names) <= set(got)
    _, g32 = Y.oracle_fp32_grads(J, P, audio, *dm, names, **oracle_kw(DEEP))
    table = Y.grad_yardstick(got, gbf, g32, names, group_of)
    print(form, "grad yardstick (d_hip, d_orc, pair, ratio):", {g: tuple(round(v, 5) for v in r.values()) for g, r in table.items()}, flush=True)
    Y.assert_grad_yardstick(table)
    # the masks matter: the oracle WITHOUT them is another function
    monkeypatch.undo()
    plain = J.jepa_forward({k: v.detach() for k, v in P.items()}, audio, *dm, mode="bf16", **oracle_kw(DEEP))
    print(form, "loss of the oracle without dropout:", float(plain["loss"]), flush=True)
    assert abs(lo - float(plain["loss"])) > 1e-3 * abs(lo)


# ------------------------------------------------------------------------------------------------------------ 2. p = 0 is the parent
def recorded_launches(monkeypatch, fn):
    from wavjepa_amd import _abi
    log = []
    real = _abi.call

    def call(name, a, stream, lab=False):
        log.append((name, int(a.drop.stream_id) if hasattr(a, "drop") else None))
        return real(name, a, stream, lab=lab)
    monkeypatch.setattr(_abi, "call", call)
    fn()
    torch.cuda.synchronize()
    monkeypatch.setattr(_abi, "call", real)
    return log


def test_a_stack_without_dropout_keeps_the_parents_launches(golden_dir, monkeypatch):
    audio, mset = draw(golden_dir)
    logs = {}
    for key, (pe, pd) in dict(none=(0.0, 0.0), enc=(P_DROP, 0.0), eval=(P_DROP, P_DROP)).items():
        m, _ = build_drop(pe, pd)
        m._ensure_engine()
        if key == "eval":
            m.eval()

        def step():
            out = m(audio, *mset)
            if key != "eval":
                out["loss"].backward()
        m(audio, *mset)                       # (first call: allocations and probes)
        logs[key] = recorded_launches(monkeypatch, step)
    names = lambda log: [n for n, _ in log]
    count = lambda log, n: names(log).count(n)
    drop_entries = ("wj_dropout_rows", "wj_layernorm_fwd_drop", "wj_layernorm_bwd_drop", "wj_attn_stream_fwd_drop", "wj_attn_stream_bwd_drop")
    assert not [n for n in names(logs["none"]) if n in drop_entries]
    L = DEEP["l_enc"]
    got = {n: count(logs["enc"], n) for n in drop_entries}
    print("launches of the _drop entries with p_enc = 0.1, p_dec = 0:", got, flush=True)
    assert got == {"wj_dropout_rows": L, "wj_layernorm_fwd_drop": 2 * L, "wj_layernorm_bwd_drop": 2 * L, "wj_attn_stream_fwd_drop": L,
                   "wj_attn_stream_bwd_drop": L}
    assert all((sid >> 16) == 0 for n, sid in logs["enc"] if sid is not None)            # every one of them the student's
    for parent, n in (("wj_attn_fwd", L), ("wj_attn_bwd", L), ("wj_layernorm_fwd", 2 * L), ("wj_layernorm_bwd", 2 * L)):
        assert count(logs["none"], parent) - count(logs["enc"], parent) == n, parent          # ... the teacher's and the predictor's stay
    others = lambda log: [n for n in names(log) if n not in drop_entries and n not in ("wj_attn_fwd", "wj_attn_bwd", "wj_layernorm_fwd",
                                                                                         "wj_layernorm_bwd")]
    assert others(logs["enc"]) == others(logs["none"])
    # an eval-mode forward of a dropout model issues exactly the launches of the dropout = 0 model's forward
    m0, _ = build_drop(0.0, 0.0)
    m0.eval()
    m0(audio, *mset)
    assert names(logs["eval"]) == names(recorded_launches(monkeypatch, lambda: m0(audio, *mset)))


def test_eval_mode_is_bit_equal_to_the_model_without_dropout(golden_dir):
    audio, mset = draw(golden_dir)
    outs = []
    for pe, pd in ((P_DROP, P_DROP), (0.0, 0.0)):
        m, _ = build_drop(pe, pd)
        m.eval()
        with torch.no_grad():
            out = m(audio, *mset)
            rep = m.get_audio_representation(audio, None)
        outs.append((bits(out["loss"].float().reshape(1)), out["preds"].clone(), out["targets"].clone(), rep.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][3]).all())


# ------------------------------------------------------------------------------------------------------------ 3. determinism
def test_masks_are_a_function_of_seed_and_call(golden_dir):
    l0, g0, m = one_step(golden_dir)
    l1, g1, _ = one_step(golden_dir)
    l_call, _, _ = one_step(golden_dir, call=1)
    l_seed, _, _ = one_step(golden_dir, dropout_seed=SEED + 1)
    l_none, _, _ = one_step(golden_dir, 0.0, 0.0)
    print("loss bits: twice", int(l0), int(l1), "other call", int(l_call), "other seed", int(l_seed), "no dropout", int(l_none), flush=True)
    assert torch.equal(l0, l1) and not differing(m, g0, g1) and torch.equal(bits(g0), bits(g1))
    assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
    assert len({int(l0), int(l_call), int(l_seed), int(l_none)}) == 4


@pytest.mark.parametrize("attrs", [{}, dict(ragged=False), dict(trim_tail=False)], ids=["ragged", "dense", "untrimmed"])
def test_recompute_regenerates_the_same_masks(golden_dir, attrs):
    l_on, g_on, m = one_step(golden_dir, attrs=attrs, use_gradient_checkpointing=True)
    l_off, g_off, _ = one_step(golden_dir, attrs=attrs)
    bad = differing(m, g_on, g_off)
    print(attrs, "loss bits on / off:", int(l_on), int(l_off), "gradient tensors that differ:", bad[:8], len(bad), flush=True)
    assert m._engine.recompute and torch.equal(l_on, l_off)
    assert not bad and torch.equal(bits(g_on), bits(g_off))


def test_checkpoint_resume_continues_the_mask_sequence(golden_dir, tmp_path):
    """6 deterministic steps against 3 steps, a checkpoint, a fresh model (another construction seed) that resumes, 3 more steps:
    parameters, moments and teacher bit for bit -- the masks of step k come from (dropout_seed, k), both of which the checkpoint holds."""
    from wavjepa_amd.trainer import Trainer
    ctx, tgt, vis = masks(golden_dir, N_CLIPS)
    batches = [(torch.from_numpy(synth.synth_audio(N_CLIPS, 1, 32159, seed=800 + i)).to(torch.bfloat16).to(dev()), ctx, tgt, vis) for i in range(6)]

    def run(root, dropout_seed, ckpt=None, skip=0):
        m, _ = build_drop(P_DROP, P_DROP, dropout_seed=dropout_seed, warmup_steps=2)
        m.on_after_batch_transfer = lambda batch, idx=0: batch                       # ready crops: the batches are pinned
        tr = Trainer(max_steps=6, default_root_dir=str(root), checkpoint_every_n_steps=3, log_every_n_steps=0, deterministic=True)
        tr.fit(m, train_dataloaders=iter(batches[skip:]), ckpt_path=ckpt)
        return m
    ma = run(tmp_path / "a", SEED)
    mb = run(tmp_path / "b", SEED + 99, ckpt=str(tmp_path / "a" / "step=3.ckpt"), skip=3)
    assert ma.global_step == mb.global_step == 6 and mb.dropout_seed == SEED and mb.hparams["dropout_seed"] == SEED
    torch.cuda.synchronize()
    for name, a, b in (("student", ma._flat.p32, mb._flat.p32), ("teacher", ma._flat.t32, mb._flat.t32),
                       ("adam_m", ma._flat.adam_m, mb._flat.adam_m), ("adam_v", ma._flat.adam_v, mb._flat.adam_v)):
        print(name, "bit-equal:", bool(torch.equal(a, b)), flush=True)
        assert torch.equal(a, b), name
    assert bool(torch.isfinite(ma._flat.p32).all())


# ------------------------------------------------------------------------------------------------------------ 4. never-written memory
def child_step(path):
    import tests.conftest as C
    l, g, _ = one_step(C.GOLDEN)
    torch.save({"loss": l.cpu(), "g32": g.cpu(), "fill": os.environ.get("WJ_ARENA_FILL", "")}, path)


def test_poisoned_arena_gives_the_same_step(golden_dir, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = tmp_path / "poisoned.pt"
    code = f"import tests.conftest; from tests import test_dropout_gpu as D; D.child_step({str(path)!r})"
    rc, out, err = launch.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, WJ_ARENA_FILL="nan"), timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    got = torch.load(path, map_location="cpu", weights_only=False)
    assert got["fill"] == "nan"
    l, g, _ = one_step(golden_dir)
    finite = bool(torch.isfinite(got["g32"]).all()) and bool(torch.isfinite(got["loss"].view(torch.float32)).all())
    print("poisoned arena: finite", finite, "loss bits", int(got["loss"]), int(l), flush=True)
    assert finite
    assert torch.equal(got["loss"], l.cpu()) and torch.equal(bits(got["g32"]), bits(g.cpu()))


# ------------------------------------------------------------------------------------------------------------ 5. the launcher
def test_launcher_trains_with_dropout(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.dropout_encoder=0.1", "trainer.size=tiny", "trainer.batch_size=1",
           "data.samples_per_audio=4", "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1", f"save_dir={tmp_path}"]
    rc, out, err = launch.run(cmd, cwd=root, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    losses = [float(v) for v in re.findall(r"step \d+\s+loss (\S+)", out)]
    print("losses:", losses, flush=True)
    assert len(losses) == 3 and all(v == v and abs(v) < float("inf") for v in losses), out[-1500:]
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    hp = ck["hyper_parameters"]
    assert ck["global_step"] == 3 and all(bool(torch.isfinite(v.float()).all()) for v in ck["state_dict"].values())
    assert hp.get("dropout_encoder") == 0.1 and hp.get("dropout_decoder") == 0.0 and isinstance(hp.get("dropout_seed"), int)


# ------------------------------------------------------------------------------------------------------------ 6. fp8
def test_fp8_mode_is_refused_with_dropout(golden_dir):
    m, _ = build_drop(P_DROP, 0.0)
    m._ensure_engine().fp8 = True
    audio, mset = draw(golden_dir)
    with pytest.raises(RuntimeError, match=r"(?s)fp8.*dropout"):
        m(audio, *mset)
