"""The collapse monitor through the engine, the module, the trainer and the launcher (GPU only): pred_var / target_var of a monitored
step against the fp64 reference of tests/moments_reference.py computed from the step's own out["preds"], out["targets"] and
target_indices, at the bound of that module (4 x the float32 two-pass yardstick on the same rows, floored at one fp32 ulp)."""
import os
import re
import sys

import pytest
import torch

from tests import launch
from tests import moments_reference as mr
from tests.test_attention_stream_gpu import clips, drawn_masks, long_model
from tests.test_dropout_gpu import recorded_launches
from tests.test_jepa_gpu import SMALL, build, dev, masks
from tests.test_prenorm_gpu import build_pre
from tests.test_recompute_gpu import bits

import synth

pytestmark = pytest.mark.gpu

N_CLIPS = 4


def draw(golden_dir, seed=3):
    audio = torch.from_numpy(synth.synth_audio(N_CLIPS, 1, 32159, seed=seed)).to(torch.bfloat16).to(dev())
    return audio, masks(golden_dir, N_CLIPS)


def assert_monitor_matches(out, tgt, eng, tag):
    """out["pred_var"] / out["target_var"] against the reference over the rows target_indices selects from the step's own tensors"""
    N, G, T = tgt.shape
    D = out["targets"].shape[-1]
    preds = out["preds"].detach().reshape(N * G * T, D).cpu()
    assert preds.dtype == torch.bfloat16
    flat = tgt.reshape(-1).to(torch.uint8).cpu()
    rows = torch.nonzero(flat).flatten().to(torch.int32)
    case = dict(B=N, G=G, T=T, D=D, preds=preds, targets=out["targets"].detach().reshape(N * T, D).float().cpu(), tgt=flat,
                dec_rows=rows, tgt_dense=rows)
    bnd = mr.bounds(case, "dense")
    ref = bnd["ref"]
    got = (float(out["pred_var"]), float(out["target_var"]))
    print(f"{tag}: n {ref['n']}  pred_var {got[0]!r} (reference {ref['pred_var']!r}, bound {bnd['bound_stat'][0]:.3e})  "
          f"target_var {got[1]!r} (reference {ref['target_var']!r}, bound {bnd['bound_stat'][1]:.3e})", flush=True)
    assert out["pred_var"].is_cuda and out["pred_var"].ndim == 0 and out["target_var"].ndim == 0
    assert float(eng.moments[2]) == ref["n"] == int(flat.sum())
    assert abs(got[0] - ref["pred_var"]) <= bnd["bound_stat"][0], tag
    assert abs(got[1] - ref["target_var"]) <= bnd["bound_stat"][1], tag
    col = eng.moments_col.cpu().numpy()
    got_cols = dict(n=ref["n"], mean=[col[0, 0], col[1, 0]], M2=[col[0, 1], col[1, 1]], pred_var=got[0], target_var=got[1])
    bad = [b for b in mr.violations(got_cols, case, "dense", bnd) if "constant column" not in b]      # (a model has no planted column)
    assert bad == [], (tag, bad)
    return ref


@pytest.mark.parametrize("form,attrs", [("ragged+trimmed", {}), ("ragged untrimmed", dict(trim_tail=False)), ("dense", dict(ragged=False))])
def test_monitored_step_matches_the_reference(golden_dir, form, attrs):
    m, _ = build(SMALL)
    eng = m._ensure_engine()
    for k, v in attrs.items():
        setattr(eng, k, v)
    m.monitor_every = 1
    audio, mset = draw(golden_dir)
    out = m(audio, *mset)
    assert eng.ragged_step == (form != "dense") and (eng.tail is not None) == (form == "ragged+trimmed")
    ref = assert_monitor_matches(out, mset[1], eng, form)
    assert ref["pred_var"] > 2e-3 and ref["target_var"] > 2e-3          # (a collapsed tensor reads sqrt(1e-6) = 1e-3)
    out["loss"].backward()                                             # the monitored step trains as any other
    assert bool(torch.isfinite(m._flat.g32).all())


def test_monitored_prenorm_step_matches_the_reference(golden_dir):
    m, _ = build_pre(SMALL)
    m.monitor_every = 1
    audio, mset = draw(golden_dir)
    out = m(audio, *mset)
    assert_monitor_matches(out, mset[1], m._engine, "pre-norm")


def test_monitored_420_token_step_matches_the_reference():
    m, _ = long_model(420)
    m.monitor_every = 1
    ctx, tgt, vis = drawn_masks(2, 420)
    out = m(clips(2, 420), ctx, tgt, vis)
    assert m._engine.T == 420
    assert_monitor_matches(out, tgt, m._engine, "420 tokens")


def test_monitor_leaves_loss_and_gradients_bit_equal(golden_dir):
    got = []
    for every in (0, 1):
        m, _ = build(SMALL)
        m._ensure_engine().deterministic = True
        m.monitor_every = every
        audio, mset = draw(golden_dir)
        out = m(audio, *mset)
        assert ("pred_var" in out) == bool(every)
        out["loss"].backward()
        torch.cuda.synchronize()
        got.append((bits(out["loss"].detach().float().reshape(1)), bits(m._flat.g32.clone())))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_launches_and_keys_follow_monitor_every(golden_dir, monkeypatch):
    audio, mset = draw(golden_dir)
    m, _ = build(SMALL)
    m._ensure_engine()
    m(audio, *mset)                               # (first call: allocations and probes)
    names = lambda log: [n for n, _ in log]
    base = names(recorded_launches(monkeypatch, lambda: m(audio, *mset)))
    assert "wj_masked_moments" not in base and m.monitor_every == 0 and m._engine.moments is None
    m.monitor_every = 2
    keys, logs = {}, {}
    for step in range(4):
        m.global_step = step
        logged = {}
        monkeypatch.setattr(m, "log_dict", lambda data, **kw: logged.update(data))
        box = {}
        log = names(recorded_launches(monkeypatch, lambda: box.update(out=m.training_step((audio, *mset), step))))
        keys[step] = ("pred_var" in box["out"], "target_var" in box["out"], "train/pred_var" in logged, "train/target_var" in logged)
        logs[step] = log
        assert log.count("wj_masked_moments") == (1 if step % 2 == 0 else 0)
        if step % 2 == 0:                         # right behind the loss
            assert log[log.index("wj_masked_moments") - 1] == "wj_masked_mse"
        assert {"train/loss", "ema"} <= set(logged)
    # nothing else of the step moves: a monitored step without its one launch is the step next to it
    assert [n for n in logs[2] if n != "wj_masked_moments"] == logs[3] == logs[1]
    assert keys == {0: (True,) * 4, 1: (False,) * 4, 2: (True,) * 4, 3: (False,) * 4}
    m.eval()                                      # an eval-mode forward is never monitored
    m.global_step = 0
    with torch.no_grad():
        assert "pred_var" not in m(audio, *mset)


def test_collapsed_predictor_is_seen_and_stops_the_trainer(golden_dir):
    from wavjepa_amd.data import SyntheticAudioSource
    from wavjepa_amd.masking import TimeInverseBlockMasker
    from wavjepa_amd.trainer import CollapseError, Trainer
    m, _ = build(SMALL, warmup_steps=2)
    with torch.no_grad():
        m.decoder_to_encoder_mapper.weight.zero_()             # every prediction is the bias: constant columns
    m.monitor_every = 1
    audio, mset = draw(golden_dir)
    out = m(audio, *mset)
    floor = float(torch.tensor(1e-6, dtype=torch.float64).sqrt().float())
    assert abs(float(out["pred_var"]) - floor) <= 1.2e-10 and float(out["target_var"]) > 2 * floor      # (one fp32 ulp of 1e-3)
    assert bool((m._engine.moments_col[0, 1] == 0).all())      # M2 of every preds column exactly 0

    src = SyntheticAudioSource(TimeInverseBlockMasker(4, 0.65, 10, 0.25, 10, 0.1), batch_size=2, samples_per_audio=2, n_tokens=200,
                               seconds=3.0, seed=11, n_mask_sets=4, device=dev())

    def loader():
        while True:
            yield src.next_batch()
    m.global_step = 0
    tr = Trainer(max_steps=6, log_every_n_steps=1, min_pred_var=0.01)
    with pytest.raises(CollapseError, match=r"pred_var = 0\.001 is below min_pred_var = 0\.01 at step 0") as e:
        tr.fit(m, train_dataloaders=loader())
    assert m.global_step == 1, "the first log step"
    print(e.value)
    m2, _ = build(SMALL, warmup_steps=2)                       # a model that has not collapsed goes through the same loop
    m2.monitor_every = 1
    Trainer(max_steps=2, log_every_n_steps=1, min_pred_var=2 * floor, min_target_var=2 * floor).fit(m2, train_dataloaders=loader())
    assert m2.global_step == 2


def test_launcher_trains_with_the_monitor(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "train.py"), "trainer.monitor_every=1", "trainer.min_pred_var=1e-6", "trainer.size=tiny",
           "trainer.batch_size=1", "data.samples_per_audio=4", "trainer.steps=3", "trainer.warmup_steps=2", "trainer.log_every_n_steps=1",
           f"save_dir={tmp_path}"]
    rc, out, err = launch.run(cmd, cwd=root, timeout=300)
    assert rc == 0, (out[-1500:], err[-4000:])
    lines = re.findall(r"step (\d+)\s+loss (\S+).*pred_var (\S+)\s+target_var (\S+) \(step (\d+)\)", out)
    print(lines, flush=True)
    assert [(int(a), int(e)) for a, _, _, _, e in lines] == [(1, 0), (2, 1), (3, 2)], out[-1500:]
    assert all(float(p) > 0 and float(t) > 0 for _, _, p, t, _ in lines)
    found = list(tmp_path.rglob("last.ckpt"))
    assert len(found) == 1
    ck = torch.load(found[0], map_location="cpu", weights_only=False)
    assert ck["global_step"] == 3 and "monitor_every" not in ck["hyper_parameters"]
