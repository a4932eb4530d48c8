"""mode="layer_norm" conv front-end, CPU side: the extractors' parameter containers against the reference's state dict, the
oracle restatement (tests/conv_layernorm_reference.py) against the reference's own outputs and gradients
(tests/golden/conv_layernorm.npz, made by tests/golden/make_conv_layernorm.py), the C ABI of the new entries, and the training
factory.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import jepa_oracle as J
from tests.conv_layernorm_reference import conv_stack_layer_norm

SPEC = [(16, 10, 5), (16, 3, 2), (16, 3, 2), (16, 2, 2)]
CASES = ("mono_bias", "mono_nobias", "chan_bias", "chan_nobias")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "conv_layernorm.npz")))


def weights(fx, case):
    pre = case + ".w."
    return {k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}


def extractor(case, **kw):
    from wavjepa_amd.extractors import ConvChannelFeatureExtractor, ConvFeatureExtractor
    kind, bias = case.split("_")
    if kind == "mono":
        return ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1, mode="layer_norm", conv_bias=bias == "bias", **kw)
    return ConvChannelFeatureExtractor(conv_layers_spec=SPEC, in_channels=2, mode="layer_norm", conv_bias=bias == "bias", **kw)


@pytest.mark.parametrize("case", CASES)
def test_state_dict_names_and_shapes_are_the_references(fixture, case):
    want = {k: tuple(v.shape) for k, v in weights(fixture, case).items()}
    ext = extractor(case)
    assert {k: tuple(v.shape) for k, v in ext.state_dict().items()} == want
    assert ext.mode == "layer_norm" and ext.conv_bias == case.endswith("_bias")
    stack = "cnn." if case.startswith("mono") else "cnns.1."
    assert (f"{stack}3.0.bias" in want) == case.endswith("_bias") and f"{stack}3.2.1.weight" in want and f"{stack}0.2.weight" not in want
    ext.load_state_dict(weights(fixture, case))           # strict


def test_refused_options_keep_raising():
    from wavjepa_amd.extractors import ConvChannelFeatureExtractor, ConvFeatureExtractor
    for cls in (ConvFeatureExtractor, ConvChannelFeatureExtractor):
        for bad in (dict(depthwise=True), dict(dropout=0.1), dict(mode="layer_norm", depthwise=True), dict(conv_bias=True)):
            with pytest.raises(NotImplementedError):
                cls(conv_layers_spec=SPEC, in_channels=1, **bad)
        with pytest.raises(ValueError):
            cls(conv_layers_spec=SPEC, in_channels=1, mode="batch_norm")
        assert "cnn.0.2.weight" in "".join(cls(conv_layers_spec=SPEC, in_channels=1).state_dict()).replace("cnns.0.", "cnn.")


# Measured on the fixture (fp32 stock torch against fp32 stock torch, relative L2): outputs <= 4.0e-7, gradients <= 1.26e-6 per tensor
# over the four cases.  Bounds: ten times that.
OUT_BOUND, GRAD_BOUND = 4.0e-6, 1.26e-5


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_reference_outputs_and_gradients(fixture, monkeypatch, case):
    monkeypatch.setattr(J, "_conv_stack", conv_stack_layer_norm)
    P = {"extract_audio." + k: v.clone().requires_grad_(True) for k, v in weights(fixture, case).items()}
    y = J.conv_frontend(P, torch.from_numpy(fixture[case + ".x"]), SPEC, "fp32")
    y.square().sum().backward()

    def rel(a, b):
        return float((a.double() - b.double()).norm() / b.double().norm())
    d_out = rel(y.detach(), torch.from_numpy(fixture[case + ".y"]))
    d_grad = {k: rel(p.grad, torch.from_numpy(fixture[f"{case}.g.{k[len('extract_audio.'):]}"])) for k, p in P.items()}
    print(case, "output", d_out, "worst gradient", max(d_grad.values()))
    assert y.shape == fixture[case + ".y"].shape
    assert d_out < OUT_BOUND, d_out
    assert max(d_grad.values()) < GRAD_BOUND, d_grad


def test_bf16_restatement_rounds_every_layer_output():
    """bf16 flow: the stack's output is a bf16 tensor (every layer's post is rounded, the last included) a bf16 step from the fp32 flow."""
    g = torch.Generator().manual_seed(3)
    P = {}
    for i, (dim, k, _) in enumerate(SPEC):
        P[f"cnn.{i}.0.weight"] = torch.randn(dim, 1 if i == 0 else dim, k, generator=g) * (2.0 / (k * (1 if i == 0 else dim))) ** 0.5
        P[f"cnn.{i}.0.bias"] = 0.02 * torch.randn(dim, generator=g)
        P[f"cnn.{i}.2.1.weight"] = 1 + 0.1 * torch.randn(dim, generator=g)
        P[f"cnn.{i}.2.1.bias"] = 0.02 * torch.randn(dim, generator=g)
    x = torch.randn(2, 1, 800, generator=g)
    y16 = conv_stack_layer_norm(P, x.to(torch.bfloat16), SPEC, "bf16", "cnn.")
    y32 = conv_stack_layer_norm(P, x.to(torch.bfloat16), SPEC, "fp32", "cnn.")
    assert y16.dtype == torch.bfloat16 and y32.dtype == torch.float32 and y16.shape == y32.shape == (2, 19, 16)
    assert float((y16.float() - y32).norm() / y32.norm()) < 2e-2


# ---------------------------------------------------------------------------------------------------------------- C ABI
NEW_STRUCTS = ("wj_conv_ln_fwd_args", "wj_conv_ln_bwd_args", "wj_conv0_ln_fwd_args", "wj_conv0_ln_bwd_args")
NEW_FUNCS = ("wj_conv_ln_gelu_fwd", "wj_conv_ln_gelu_bwd", "wj_conv_ln_bwd_partial_rows", "wj_conv0_ln_gelu_fwd", "wj_conv0_ln_gelu_bwd")


def test_abi_version_stays_17_and_new_structs_match():
    from wavjepa_amd import _abi
    lib = _abi.load()
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 and lib.wj_abi_version() == 17
    for name in NEW_STRUCTS:
        assert lib.wj_struct_size(name.encode()) == ctypes.sizeof(_abi.STRUCTS[name]) > 0
    for fn in NEW_FUNCS:
        assert fn in _abi.FUNCTIONS and hasattr(lib, fn)


def test_partial_row_and_workspace_queries_agree():
    from wavjepa_amd import ops
    for rows, C in ((0, 64), (1, 64), (120, 64), (5000, 512), (823168, 512), (3, 128), (77, 256)):
        n = ops.conv_ln_bwd_partial_rows(rows, C)
        assert 1 <= n <= 1536
        assert ops.workspace_bytes("wj_conv_ln_gelu_bwd", M=rows, C=C) == n * 3 * C * 4
        # the engine's reduction scratch and fold slots are sized by wj_layernorm_bwd's query: the partial rows must fit them
        assert n * 3 * C * 4 <= ops.workspace_bytes("wj_layernorm_bwd", D=C)
    for rows, C in ((-1, 64), (8, 96), (8, 1024), (8, 0)):
        assert ops.conv_ln_bwd_partial_rows(rows, C) == -1
    dims = dict(N=3, C_in=1, C=64, k=10, L_out=162)
    rec = 64 * (10 + 3) * 4
    dense = ops.workspace_bytes("wj_conv0_ln_gelu_bwd", max_rows=0, **dims)
    assert dense == 3 * (1 + 1) * rec
    assert ops.workspace_bytes("wj_conv0_ln_gelu_bwd", max_rows=513, **dims) == 3 * (1 + 2) * rec
    assert ops.workspace_bytes("wj_conv0_ln_gelu_bwd", max_rows=40, **dims) <= dense      # a listed step fits the dense scratch
    assert ops.workspace_bytes("wj_conv0_ln_gelu_bwd", **dict(dims, C_in=2, C=512, L_out=6431)) == 3 * (1 + 13) * 512 * 23 * 4
    from wavjepa_amd import _abi
    lib = _abi.load()
    for fn in ("wj_conv_ln_gelu_fwd", "wj_conv0_ln_gelu_fwd"):
        assert lib.wj_workspace_bytes(fn.encode(), b"x") == 0
    a = _abi.STRUCTS["wj_conv0_ln_bwd_args"](N=0, C_in=1, C=64, k=10, L_out=162)
    assert lib.wj_workspace_bytes(b"wj_conv0_ln_gelu_bwd", ctypes.byref(a)) == -1


def test_new_entries_validate_their_arguments_before_any_launch():
    """NULL or short arguments return WJ_ERR_ARG (-1), an unsupported width or tap count WJ_ERR_UNSUPPORTED (-3), without touching a
    device: the pointers below are never dereferenced."""
    from wavjepa_amd import _abi
    lib = _abi.load()
    fake = 1 << 20

    def call(fn, struct, base, **kw):
        a = _abi.STRUCTS[struct](**dict(base, **kw))
        return getattr(lib, fn)(ctypes.byref(a), None)

    fwd = dict(pre=fake, gamma=fake, beta=fake, post=fake, mean=fake, rstd=fake, M=120, C=64, seg_rows=40, seg_valid=37, eps=1e-5)
    bwd = dict(dpost=fake, pre=fake, mean=fake, rstd=fake, gamma=fake, beta=fake, dpre=fake, workspace=fake, M=120, C=64, seg_rows=40,
               seg_valid=37)
    geo = dict(N=3, C_in=1, L=815, C=64, k=10, stride=5, L_out=162, P=168)
    fwd0 = dict(geo, audio=fake, w=fake, bias=fake, gamma=fake, beta=fake, act=fake, mean=fake, rstd=fake, eps=1e-5)
    bwd0 = dict(geo, audio=fake, w=fake, bias=fake, gamma=fake, beta=fake, mean=fake, rstd=fake, dact=fake, dw=fake, dbias=fake, dgamma=fake,
                dbeta=fake, workspace=fake)
    table = (("wj_conv_ln_gelu_fwd", "wj_conv_ln_fwd_args", fwd,
              [dict(pre=None), dict(gamma=None), dict(beta=None), dict(post=None), dict(M=0), dict(C=0), dict(seg_valid=0), dict(seg_valid=41),
               dict(pre=fake + 2)], [dict(C=96), dict(C=1024), dict(C=16)]),
             ("wj_conv_ln_gelu_bwd", "wj_conv_ln_bwd_args", bwd,
              [dict(dpost=None), dict(pre=None), dict(mean=None), dict(rstd=None), dict(gamma=None), dict(beta=None), dict(dpre=None),
               dict(workspace=None), dict(M=-1), dict(rows=fake, n_rows=-1), dict(seg_rows=-2)], [dict(C=96), dict(C=768)]),
             ("wj_conv0_ln_gelu_fwd", "wj_conv0_ln_fwd_args", fwd0,
              [dict(audio=None), dict(w=None), dict(gamma=None), dict(act=None), dict(mean=None), dict(rstd=None), dict(N=0), dict(P=161),
               dict(L=814), dict(stride=0), dict(audio_clip_stride=800)], [dict(C=96), dict(k=9), dict(C_in=3)]),
             ("wj_conv0_ln_gelu_bwd", "wj_conv0_ln_bwd_args", bwd0,
              [dict(audio=None), dict(dact=None), dict(dw=None), dict(dgamma=None), dict(dbeta=None), dict(workspace=None), dict(mean=None),
               dict(L=814), dict(rows=fake, row_off=None), dict(rows=fake, row_off=fake, max_rows=-1), dict(dbias=None), dict(bias=None)],
              [dict(C=96), dict(k=7)]))
    for fn, struct, base, args_bad, unsupported in table:
        assert getattr(lib, fn)(None, None) == -1, fn
        for bad in args_bad:
            assert call(fn, struct, base, **bad) == -1, (fn, bad)
        for bad in unsupported:
            assert call(fn, struct, base, **bad) == -3, (fn, bad)


# ---------------------------------------------------------------------------------------------------------------- host side
@pytest.mark.parametrize("name", ["wavjepa", "wavjepa_nat"])
def test_training_factory_passes_mode_and_conv_bias(name):
    import train
    from wavjepa_amd.config import load_config
    over = [f"extractor={name}"] + (["data=nat_synthetic", "masker=AudioSet_nat"] if name == "wavjepa_nat" else [])
    cfg = load_config(os.path.join(ROOT, "configs"), over)
    ext = train.ComponentFactory.create_extractor(cfg)
    assert ext.mode == "default" and ext.conv_bias is False
    cfg = load_config(os.path.join(ROOT, "configs"), over + ["extractor.mode=layer_norm", "extractor.conv_bias=true"])
    ext = train.ComponentFactory.create_extractor(cfg)
    assert ext.mode == "layer_norm" and ext.conv_bias is True
    sd = ext.state_dict()
    stack = "cnn." if name == "wavjepa" else "cnns.1."
    assert sd[f"{stack}5.0.bias"].shape == (512,) and sd[f"{stack}0.2.1.weight"].shape == (512,)


def test_denoiser_refuses_the_mode_and_engine_config_defaults():
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.engine import EngineConfig
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    cfg = EngineConfig(conv_spec=SPEC, in_channels=1, n_samples=800, d_enc=64, h_enc=2, l_enc=1, d_dec=64, h_dec=2, l_dec=1, top_k=1)
    assert cfg.conv_mode == "default" and cfg.conv_bias is False
    ext = ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1, mode="layer_norm", conv_bias=True)
    with pytest.raises(NotImplementedError, match="default conv front-end"):
        Denoiser(ext, TransformerLayerCFG.create(d_model=64, nhead=2), TransformerEncoderCFG.create(num_layers=1))
