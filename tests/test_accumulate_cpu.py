"""Gradient accumulation (accumulate_grad_batches) on the host: the reference composition of tests/accumulate_reference.py against the
oracle's own train_step, the trainer's argument, the launcher's key, the micro-batch / dropout-counter arithmetic, the checkpoint keys
and the Denoiser refusal.  The accumulated step itself is checked on the GPU (tests/test_accumulate_gpu.py)."""
import inspect
import os
import types

import pytest
import torch

from oracle import jepa_oracle as J
from tests import accumulate_reference as A
from tests.test_host_cpu import small_model
from tests.test_oracle_golden import TINY, load, params_from, rel
from tests.test_recompute_cpu import DEFAULT_HPARAMS, plain_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHORT = dict(warmup=3, total_steps=20, ema=(0.9, 0.99, 10))


def tiny(golden_dir):
    fx, masks = load(golden_dir, "tiny_traj.npz"), load(golden_dir, "masks.npz")
    batches = []
    for j in range(3):
        sl = slice(2 * j, 2 * j + 2)
        batches.append((torch.from_numpy(fx["audio"][j]),) + tuple(torch.from_numpy(masks[k][sl]) for k in ("as_ctx", "as_tgt", "as_vis")))
    return (lambda: params_from(fx, "sd0::")), batches


# ------------------------------------------------------------------------------------------------------------ the reference helper
def test_helper_at_k_1_is_the_oracles_train_step(golden_dir):
    fresh, batches = tiny(golden_dir)
    Pa, Pb, sa, sb = fresh(), fresh(), {}, {}
    for i in range(3):
        a = A.train_window(Pa, sa, i, [batches[i]], mode="fp32", **SHORT, **TINY)
        b = J.train_step(Pb, sb, i, batches[i], mode="fp32", **SHORT, **TINY)
        assert a["losses"] == [b["loss"]] and a["loss"] == b["loss"] and a["grad_norm"] == b["grad_norm"] and a["ema"] == b["ema"]
    assert set(Pa) == set(Pb)
    for n in Pa:
        assert torch.equal(Pa[n], Pb[n]), n
    for n in sa:
        assert torch.equal(sa[n]["m"], sb[n]["m"]) and torch.equal(sa[n]["v"], sb[n]["v"]), n


def test_helper_at_k_2_with_one_batch_fed_twice_is_k_1_on_that_batch(golden_dir):
    fresh, batches = tiny(golden_dir)
    P2, P1 = fresh(), fresh()
    two = A.train_window(P2, {}, 1, [batches[0], batches[0]], mode="fp32", **SHORT, **TINY)
    one = A.train_window(P1, {}, 1, [batches[0]], mode="fp32", **SHORT, **TINY)
    # the second forward sees the teacher after one EMA: its targets, loss and gradient differ from the first one's by what the EMA
    # moved -- so compare with the EMA held still (ema = (1, 1, n): r = 1 leaves the teacher where it is), and the EMA on its own
    assert two["losses"][0] == one["losses"][0] and two["losses"][1] != one["losses"][0]
    still = dict(SHORT, ema=(1.0, 1.0, 10))
    P2, P1 = fresh(), fresh()
    two = A.train_window(P2, {}, 1, [batches[0], batches[0]], mode="fp32", **still, **TINY)
    one = A.train_window(P1, {}, 1, [batches[0]], mode="fp32", **still, **TINY)
    assert two["losses"] == [one["loss"], one["loss"]] and two["loss"] == one["loss"]
    assert abs(two["grad_norm"] - one["grad_norm"]) <= 1e-6 * one["grad_norm"]
    worst = max(rel(P2[n], P1[n]) for n in J.trainable_names(P1))
    print("k = 2 on one batch twice against k = 1: worst relative parameter distance", worst)
    assert worst <= 1e-6
    # the EMA: two applications per optimiser step against one -- r^2 on the teacher
    r = J.ema_decay(1, *SHORT["ema"])
    Pe, P0 = fresh(), fresh()
    J.ema_update(Pe, r)
    J.ema_update(Pe, r)
    for n in P0:
        if n.startswith("teacher_encoder."):
            want = r * r * P0[n].double() + (1 - r * r) * P0[n[len("teacher_"):]].double()
            assert rel(Pe[n], want) <= 1e-6, n
    Pk = fresh()
    A.train_window(Pk, {}, 1, [batches[0], batches[0]], mode="fp32", **SHORT, **TINY)
    for n in Pk:
        if n.startswith("teacher_encoder."):
            assert torch.equal(Pk[n], Pe[n]), n


def test_helper_keeps_the_scale_when_the_window_is_short(golden_dir):
    fresh, batches = tiny(golden_dir)
    Pa, Pb = fresh(), fresh()
    part = A.train_window(Pa, {}, 0, [batches[0]], 2, mode="fp32", clip=1e9, **SHORT, **TINY)
    full = A.train_window(Pb, {}, 0, [batches[0]], 1, mode="fp32", clip=1e9, **SHORT, **TINY)
    assert abs(part["grad_norm"] - full["grad_norm"] / 2) <= 1e-6 * full["grad_norm"]


# ------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_stores_and_checks_the_argument():
    from wavjepa_amd.jepa import accumulate_window
    from wavjepa_amd.trainer import StepRunner, Trainer
    assert inspect.signature(Trainer.__init__).parameters["accumulate_grad_batches"].default == 1
    assert Trainer().accumulate_grad_batches == 1
    assert Trainer(accumulate_grad_batches=1).accumulate_grad_batches == 1
    t = Trainer(accumulate_grad_batches=3)
    assert t.accumulate_grad_batches == 3
    for bad in (0, -1, 2.5, "2", True, None):
        with pytest.raises(ValueError, match="accumulate_grad_batches"):
            Trainer(accumulate_grad_batches=bad)
    m = small_model()
    assert accumulate_window(m) == 1              # (no trainer attached: one loader batch per optimiser step)
    m.trainer = t
    assert m.trainer.accumulate_grad_batches == 3 and accumulate_window(m) == 3
    # positional use by the benchmark is unchanged: the new argument comes last
    assert list(inspect.signature(StepRunner.__init__).parameters)[1:] == ["model", "gradient_clip_val", "enc_chunk", "accumulate_grad_batches"]
    assert inspect.signature(StepRunner.__init__).parameters["accumulate_grad_batches"].default == 1


def test_launcher_passes_the_key_on():
    import denoise
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(ROOT, "configs")
    assert train.setup_trainer(load_config(root, ["trainer.size=tiny"])).accumulate_grad_batches == 1
    assert train.setup_trainer(load_config(root, ["trainer.size=tiny", "trainer.accumulate_grad_batches=4"])).accumulate_grad_batches == 4
    with pytest.raises(ValueError, match="accumulate_grad_batches"):
        train.setup_trainer(load_config(root, ["trainer.accumulate_grad_batches=0"]))
    assert 'cfg.trainer.get("accumulate_grad_batches", 1)' in inspect.getsource(train)
    assert denoise.setup_trainer(load_config(root, [], config_name="denoise")).accumulate_grad_batches == 1
    assert denoise.setup_trainer(load_config(root, ["trainer.accumulate_grad_batches=2"], config_name="denoise")).accumulate_grad_batches == 2


# ------------------------------------------------------------------------------------------------------------ counters
def test_micro_index_and_dropout_counter():
    from wavjepa_amd.jepa import dropout_call_of
    for gs in (0, 1, 7, 374999):
        assert dropout_call_of(gs) == dropout_call_of(gs, 1, 0) == A.dropout_call(gs, 1, 0) == gs
        for i in range(3):
            assert dropout_call_of(gs, 3, i) == A.dropout_call(gs, 3, i) == 3 * gs + i
    # consecutive micro-batches of consecutive steps never share a counter
    seen = [dropout_call_of(gs, 3, i) for gs in range(5) for i in range(3)]
    assert seen == list(range(15))
    assert dropout_call_of(9, 3, 1, explicit=5) == A.dropout_call(9, 3, 1, 5) == 5 and dropout_call_of(9, 1, 0, explicit=0) == 0
    top = (1 << 32) - 1
    assert dropout_call_of(top // 3, 3, top % 3) == A.dropout_call(top // 3, 3, top % 3) == top
    for fn in (dropout_call_of, A.dropout_call):
        with pytest.raises(OverflowError):
            fn(top // 3 + 1, 3, 0)
        with pytest.raises(OverflowError):
            fn(1 << 31, 2, 0)
    with pytest.raises(ValueError):
        dropout_call_of(0, 3, 3)
    assert [A.micro_index(b, 3) for b in range(7)] == [0, 1, 2, 0, 1, 2, 0]


def test_training_step_sets_the_micro_index_for_its_forward_only():
    m = small_model()
    assert m.accumulate_grads is False and m._micro == (0, 1)
    seen = []
    m.log_dict = lambda data, **kw: None
    m._step_teacher = lambda: None
    m.forward = lambda *a: seen.append(m._micro) or dict(loss=torch.tensor(1.0))
    for b in range(3):
        m.training_step((None, None, None, None), b)
    m.trainer = types.SimpleNamespace(accumulate_grad_batches=3, max_steps=10)
    for b in range(5):
        m.training_step((None, None, None, None), b)
    assert seen == [(0, 1)] * 3 + [(0, 3), (1, 3), (2, 3), (0, 3), (1, 3)]
    assert m._micro == (0, 1)


# ------------------------------------------------------------------------------------------------------------ module surface
def test_default_models_surface_is_what_it_was():
    from wavjepa_amd.engine import JepaEngine
    from wavjepa_amd.jepa import JEPA
    m = small_model()
    assert m.accumulate_grads is False
    if plain_path():
        assert set(m.hparams) == DEFAULT_HPARAMS
    ctor = set(inspect.signature(JEPA.__init__).parameters)
    assert not {p for p in ctor if "accumulate" in p} and not {h for h in m.hparams if "accumulate" in h}
    assert inspect.signature(JepaEngine.backward).parameters["accumulate"].default is False
    assert list(inspect.signature(JepaEngine.backward).parameters)[:3] == ["self", "gscale_ptr", "on_grads_ready"]
    # zero_grad() without the flag: the no-op it was (no engine exists on this host: a clear would have to build one)
    opt = m.configure_optimizers()["optimizer"]
    assert opt.zero_grad() is None and m._engine is None


# ------------------------------------------------------------------------------------------------------------ checkpoints
class _Runner:
    def __init__(self):
        self.optimizer = types.SimpleNamespace(state_dict=lambda: dict(step=0))
        self.scheduler = types.SimpleNamespace(state_dict=lambda: dict(last_epoch=0))


def test_checkpoint_carries_the_key_only_above_1(tmp_path):
    from wavjepa_amd.trainer import Trainer, saved_accumulate
    m = small_model()
    usual = {"state_dict", "hyper_parameters", "global_step", "optimizer", "lr_scheduler"}
    for k in (1, 2):
        path = str(tmp_path / f"k{k}.ckpt")
        Trainer(accumulate_grad_batches=k).save_checkpoint(m, _Runner(), path)
        ck = torch.load(path, map_location="cpu", weights_only=False)
        assert set(ck) == (usual if k == 1 else usual | {"accumulate_grad_batches"})
        assert saved_accumulate(ck) == k and "accumulate_grad_batches" not in ck["hyper_parameters"]
    # a hand-built checkpoint without the key (every checkpoint from before, the reference's): reads as k = 1
    path = str(tmp_path / "hand.ckpt")
    torch.save({"state_dict": {n: v.clone() for n, v in m.state_dict().items()}, "global_step": 5}, path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    assert saved_accumulate(ck) == 1
    small_model().load_state_dict(ck["state_dict"])


# ------------------------------------------------------------------------------------------------------------ the Denoiser stage
def test_denoiser_is_refused_on_the_host():
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.trainer import StepRunner, Trainer
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    den = Denoiser(ConvFeatureExtractor(conv_layers_spec=[(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)], in_channels=1),
                   TransformerLayerCFG.create(d_model=64, nhead=2), TransformerEncoderCFG.create(num_layers=1))
    moved = []
    den.to = lambda *a, **k: moved.append(a)         # the first thing fit() does on the GPU
    den._ensure_engine = lambda: moved.append("engine")

    def loader():
        moved.append("loader")
        yield None
    with pytest.raises(NotImplementedError, match=r"accumulate_grad_batches=2.*Denoiser"):
        Trainer(accumulate_grad_batches=2).fit(den, train_dataloaders=loader())
    with pytest.raises(NotImplementedError, match=r"accumulate_grad_batches=3.*Denoiser"):
        StepRunner(den, 1.0, accumulate_grad_batches=3)
    assert not moved
