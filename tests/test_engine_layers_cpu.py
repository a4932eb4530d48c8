"""The layering of the step engines: an encoder base (encoder_engine.EncoderEngine) under the JEPA and the denoiser step, the upload
plumbing and the mask plan in modules of their own, every name that was imported from wavjepa_amd.engine still importable from it.
No GPU: classes, signatures and sources only."""
import importlib
import inspect
import re

SPEC = [(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)]


def test_both_step_engines_stand_on_the_encoder_base():
    from wavjepa_amd.denoiser import DenoiserEngine
    from wavjepa_amd.encoder_engine import EncoderEngine
    from wavjepa_amd.engine import JepaEngine
    assert issubclass(DenoiserEngine, EncoderEngine) and issubclass(JepaEngine, EncoderEngine)
    assert not issubclass(DenoiserEngine, JepaEngine)
    # the base is written over the set of trainable stacks: "enc" always, the JEPA step adds "dec"
    assert set(EncoderEngine.BW_RING) == set(DenoiserEngine.BW_RING) == {"enc"} and set(JepaEngine.BW_RING) == {"enc", "dec"}
    assert "_bind_params" not in vars(DenoiserEngine)
    assert list(inspect.signature(JepaEngine.__init__).parameters) == ["self", "cfg", "flat", "pos_enc", "pos_dec"]
    assert list(inspect.signature(DenoiserEngine.__init__).parameters) == ["self", "cfg", "flat", "pos_enc"]


def test_engine_config_builds_without_the_predictor_fields():
    from wavjepa_amd.encoder_engine import EngineConfig
    cfg = EngineConfig(conv_spec=SPEC, in_channels=1, n_samples=32159, d_enc=128, h_enc=2, l_enc=2)
    assert (cfg.d_dec, cfg.h_dec, cfg.l_dec, cfg.top_k) == (0, 0, 0, 1)
    names = list(EngineConfig.__dataclass_fields__)
    assert names[:11] == ["conv_spec", "in_channels", "n_samples", "d_enc", "h_enc", "l_enc", "d_dec", "h_dec", "l_dec", "top_k", "streams"]


def test_engine_keeps_every_name_imported_from_it():
    from wavjepa_amd import conv_frontend, encoder_engine, engine, mask_plan, upload
    for name in ("EngineConfig", "JepaEngine", "MaskPlan", "make_mask_plan", "pack_upload", "_layer_ptrs", "_upload_stream",
                 "_UPLOAD_STREAMS", "conv_geometry", "conv_active_rows", "ConvFrontend", "ConvLayerParams", "_empty"):
        assert hasattr(engine, name), name
    assert engine._UPLOAD_STREAMS is upload._UPLOAD_STREAMS
    assert engine.pack_upload is upload.pack_upload and engine._upload_stream is upload._upload_stream
    assert engine.MaskPlan is mask_plan.MaskPlan and engine.make_mask_plan is mask_plan.make_mask_plan
    assert engine.EngineConfig is encoder_engine.EngineConfig and engine.ConvFrontend is conv_frontend.ConvFrontend


def test_upload_users_import_it_directly():
    from wavjepa_amd import audio_prep, conv_frontend, jepa, upload
    assert "upload" not in inspect.signature(conv_frontend.ConvFrontend.__init__).parameters
    assert conv_frontend.pack_upload is upload.pack_upload and jepa.pack_upload is upload.pack_upload
    assert audio_prep._upload_stream is upload._upload_stream
    src = inspect.getsource(audio_prep)
    assert not re.search(r"^\s+(from|import)\s+\S*engine", src, re.M)       # no function-local import of the engine
    assert "__import__" not in inspect.getsource(upload)


def test_engine_state_is_declared_where_its_owner_is_built():
    from wavjepa_amd import params
    init = inspect.getsource(params.FlatParams.__init__)
    assert re.search(r"self\.g_clean\s*=\s*False", init)
    for module in ("encoder_engine", "engine", "denoiser", "jepa"):
        src = inspect.getsource(importlib.import_module("wavjepa_amd." + module))
        for name in ("cap_enc", "_train_alloc", "_opt_main", "g_clean", "dn_loss"):
            assert not re.search(r"(getattr|hasattr)\(\w+(\.\w+)*, \"%s\"" % name, src), (module, name)
