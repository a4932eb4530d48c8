"""Activation recomputation (JEPA use_gradient_checkpointing -> EngineConfig.recompute) on the host: the module surface, the
hyper-parameters a checkpoint records, the launcher's key and the engine configuration's default.  The step itself is checked on
the GPU (tests/test_recompute_gpu.py)."""
import os

from tests.test_host_cpu import small_model

# what a default model has always recorded on the plain (no Lightning) path: the constructor's scalar arguments
DEFAULT_HPARAMS = {"lr", "adam_betas", "adam_eps", "adam_weight_decay", "ema_decay", "ema_end_decay", "ema_anneal_end_step",
                   "average_top_k_layers", "resample_sr", "process_audio_seconds", "nr_samples_per_audio", "compile_modules", "size",
                   "warmup_steps", "decoder_embedding_dim"}


def plain_path():
    from wavjepa_amd import jepa
    return not jepa.HAS_LIGHTNING


def test_attribute_follows_the_argument():
    assert small_model().use_gradient_checkpointing is False
    assert small_model(use_gradient_checkpointing=False).use_gradient_checkpointing is False
    assert small_model(use_gradient_checkpointing=True).use_gradient_checkpointing is True
    assert small_model(use_gradient_checkpointing=1).use_gradient_checkpointing is True


def test_hparams_record_the_flag_only_when_it_is_set():
    if not plain_path():     # Lightning's save_hyperparameters records every constructor argument, as the reference does
        assert small_model().hparams["use_gradient_checkpointing"] is False
        assert small_model(use_gradient_checkpointing=True).hparams["use_gradient_checkpointing"] is True
        return
    base = small_model()
    assert "use_gradient_checkpointing" not in base.hparams
    assert "use_gradient_checkpointing" not in small_model(use_gradient_checkpointing=False).hparams
    m = small_model(use_gradient_checkpointing=True)
    assert m.hparams["use_gradient_checkpointing"] is True
    assert set(m.hparams) == set(base.hparams) | {"use_gradient_checkpointing"}


def test_default_models_checkpoint_hyper_parameters_are_what_they_were():
    m = small_model()
    saved = dict(m.hparams)                          # what Trainer.save_checkpoint writes as "hyper_parameters"
    if plain_path():
        assert set(saved) == DEFAULT_HPARAMS
    else:                    # Lightning's save_hyperparameters: every constructor argument but the ignored modules, as the reference
        assert DEFAULT_HPARAMS <= set(saved) and saved["use_gradient_checkpointing"] is False
    assert saved["size"] == "base" and saved["compile_modules"] is False and saved["average_top_k_layers"] == 2


def test_launcher_reads_the_key():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    tiny = ["trainer.size=tiny"]
    assert load_config(root, tiny).trainer.get("use_gradient_checkpointing", False) is False
    off, _ = train.build_model(load_config(root, tiny))
    on, _ = train.build_model(load_config(root, tiny + ["trainer.use_gradient_checkpointing=true"]))
    assert off.use_gradient_checkpointing is False and on.use_gradient_checkpointing is True
    if plain_path():
        assert "use_gradient_checkpointing" not in off.hparams and on.hparams["use_gradient_checkpointing"] is True


def test_engine_config_default_and_field():
    from wavjepa_amd.engine import EngineConfig, JepaEngine
    fields = {f.name: f.default for f in EngineConfig.__dataclass_fields__.values()}
    assert fields["recompute"] is False
    # the rings of the recomputed activations are the backward's own: one place defines their slot counts
    assert JepaEngine.BW_RING == dict(enc=(4, 2), dec=(2, 1))
