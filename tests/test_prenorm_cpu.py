"""CPU tests of the pre-norm (norm_first=True) surface: the test reference against PyTorch's own TransformerEncoder, the module
surface (construction, state_dict layout, the Denoiser's refusal) and the C ABI of the two new LayerNorm entries (struct layout,
argument validation) -- none of it needs a GPU."""
import ctypes

import pytest
import torch
from torch import nn

from oracle import jepa_oracle as J
from tests import prenorm_reference as R

SPEC = [(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)]


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _torch_stack(d, h, layers, eps):
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=h, dim_feedforward=4 * d, dropout=0.0, activation="gelu", layer_norm_eps=eps,
                                       batch_first=True, norm_first=True)
    enc = nn.TransformerEncoder(layer, num_layers=layers, norm=nn.LayerNorm(d), enable_nested_tensor=False)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():            # (nn.TransformerEncoder deep-copies one layer: give every parameter its own values)
        for n, p in enc.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.2 if p.ndim == 2 else 0.1))
            if "norm" in n and n.endswith("weight"):
                p.add_(1.0)
    return enc.train()               # train mode: the plain Python path, never the fused inference fast path


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_pre_norm_reference_equals_torch_transformer_encoder(layers, masked):
    """The helper's layer (1) and three-layer stack (3, with the final norm) against nn.TransformerEncoder(norm_first=True) in fp32 with
    the same weights, with and without a key-padding mask.  1e-5 relative L2: fp32 round-off of two formulations of one arithmetic."""
    d, h, eps = 64, 4, 1e-6
    enc = _torch_stack(d, h, layers, eps)
    P = {f"stack.{k}": v.detach() for k, v in enc.state_dict().items()}
    x = torch.randn(3, 37, d, generator=torch.Generator().manual_seed(1))
    mask = None
    if masked:
        mask = torch.zeros(3, 37, dtype=torch.bool)
        mask[0, 30:] = True
        mask[2, ::3] = True
    with torch.no_grad():
        want = enc(x, src_key_padding_mask=mask)
        if layers == 1:
            got = R.pre_norm_layer(P, "stack.layers.0.", x, h, mask, "fp32", eps)
            got = J._ln(got, P["stack.norm.weight"], P["stack.norm.bias"], 1e-5)
        else:
            got = x
            for i in range(layers):
                got = R.pre_norm_layer(P, f"stack.layers.{i}.", got, h, mask, "fp32", eps)
            got = J._ln(got, P["stack.norm.weight"], P["stack.norm.bias"], 1e-5)
    assert rel(got, want) < 1e-5, rel(got, want)


def test_monkeypatched_oracle_stack_is_the_pre_norm_stack(monkeypatch):
    """J.encoder_stack under the monkeypatch == nn.TransformerEncoder(norm_first=True); the mixed variant switches by prefix."""
    d, h, eps = 64, 4, 1e-6
    enc = _torch_stack(d, h, 3, eps)
    P = {f"encoder.{k}": v.detach() for k, v in enc.state_dict().items()}
    P.update({f"decoder.{k}": v.detach() for k, v in enc.state_dict().items()})
    x = torch.randn(2, 21, d, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        want = enc(x)
        post = J.encoder_stack(P, "encoder", x, h, None, "fp32", eps=eps)
        monkeypatch.setattr(J, "post_norm_layer", R.pre_norm_layer)
        assert rel(J.encoder_stack(P, "encoder", x, h, None, "fp32", eps=eps), want) < 1e-5
        monkeypatch.setattr(J, "post_norm_layer", R.mixed_layer(R.PREDICTOR))
        assert rel(J.encoder_stack(P, "decoder", x, h, None, "fp32", eps=eps), want) < 1e-5
        assert torch.equal(J.encoder_stack(P, "encoder", x, h, None, "fp32", eps=eps), post)
    assert rel(post, want) > 1e-2            # (the two layouts are different functions of the same weights)


def _jepa(enc_first=False, dec_first=False, **kw):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    return JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1),
                transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=2),
                transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2, norm_first=enc_first),
                transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=2),
                transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=32, nhead=2, norm_first=dec_first),
                average_top_k_layers=2, process_audio_seconds=2.01, nr_samples_per_audio=2, **kw)


def test_pre_norm_jepa_constructs_with_the_post_norm_state_dict_layout():
    """norm_first=True constructs on a CPU-only host; names and shapes of the state dict are the post-norm model's, and each loads
    into the other.  The flags reach the checkpoint's hyper-parameters only when set."""
    post, pre = _jepa(), _jepa(True, True)
    sp, sq = post.state_dict(), pre.state_dict()
    assert list(sp) == list(sq)
    assert {k: tuple(v.shape) for k, v in sp.items()} == {k: tuple(v.shape) for k, v in sq.items()}
    pre.load_state_dict(sp)
    post.load_state_dict(sq)
    assert all(torch.equal(pre.state_dict()[k], sp[k]) for k in sp)
    assert pre.encoder.norm_first and pre.decoder.norm_first and pre.teacher_encoder.norm_first
    assert not post.encoder.norm_first and not post.decoder.norm_first
    assert pre.hparams["norm_first_encoder"] is True and pre.hparams["norm_first_decoder"] is True
    assert "norm_first_encoder" not in post.hparams and "norm_first_decoder" not in post.hparams
    only_dec = _jepa(False, True)
    assert "norm_first_encoder" not in only_dec.hparams and only_dec.hparams["norm_first_decoder"] is True
    assert not only_dec.teacher_encoder.norm_first


def test_unsupported_layer_configs_keep_raising():
    from wavjepa_amd.jepa import TransformerStack
    from wavjepa_amd.types import TransformerLayerCFG
    with pytest.raises(NotImplementedError):
        TransformerStack(dict(TransformerLayerCFG.create(d_model=64, nhead=2, norm_first=True), dropout=0.1), 1)
    with pytest.raises(NotImplementedError):
        TransformerStack(dict(TransformerLayerCFG.create(d_model=64, nhead=2, norm_first=True), dim_feedforward=128), 1)


def test_denoiser_refuses_a_pre_norm_config():
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    with pytest.raises(NotImplementedError, match="Denoiser"):
        Denoiser(ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1),
                 TransformerLayerCFG.create(d_model=64, nhead=2, norm_first=True), TransformerEncoderCFG.create(num_layers=1))


def test_hear_runtime_takes_norm_first():
    from hear_api.runtime import RuntimeJEPA
    from wavjepa_amd.extractors import ConvFeatureExtractor
    rt = RuntimeJEPA(in_channels=1, weights=None, is_spectrogram=False, process_seconds=2.01,
                     extractor=ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1), model_size="tiny", sr=16000, norm_first=True)
    assert rt.model.encoder.norm_first and rt.model.decoder.norm_first


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_version_and_new_struct_layouts():
    from wavjepa_amd import _abi
    lib = _abi.load()                # (cross-checks every struct of the header against wj_struct_size)
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 and lib.wj_abi_version() == 17
    for name in ("wj_ln_pre_fwd_args", "wj_ln_pre_bwd_args"):
        assert lib.wj_struct_size(name.encode()) == ctypes.sizeof(_abi.STRUCTS[name]) > 0
    for fn in ("wj_layernorm_pre_fwd", "wj_layernorm_pre_bwd", "wj_ln_pre_bwd_partial_rows"):
        assert fn in _abi.FUNCTIONS and hasattr(lib, fn)


def test_partial_row_and_workspace_queries():
    from wavjepa_amd import ops
    for M, D in ((1, 64), (400, 768), (16391, 768), (32775, 384), (51200, 768)):
        rows = ops.ln_pre_bwd_partial_rows(M, D)
        assert rows == ops.ln_bwd_partial_rows(M, D) and 1 <= rows <= 1536
        assert ops.workspace_bytes("wj_layernorm_pre_bwd", M=M, D=D) >= rows * 3 * D * 4
    assert ops.ln_pre_bwd_partial_rows(0, 64) == -1
    assert ops.workspace_bytes("wj_layernorm_pre_bwd", D=768) == 1536 * 3 * 768 * 4


def test_new_entries_validate_their_arguments_before_any_launch():
    """NULL x / gamma (beta, s, dy, mean, rstd), an unsupported D and group_stats without group_rows return WJ_ERR_ARG (-1) without
    touching a device: the pointers below are never dereferenced."""
    from wavjepa_amd import _abi
    lib = _abi.load()
    fake = 1 << 20

    def fwd(**kw):
        a = _abi.STRUCTS["wj_ln_pre_fwd_args"](**dict(dict(x=fake, gamma=fake, beta=fake, y_bf16=fake, M=8, D=64, eps=1e-6), **kw))
        return lib.wj_layernorm_pre_fwd(ctypes.byref(a), None)

    def bwd(**kw):
        a = _abi.STRUCTS["wj_ln_pre_bwd_args"](**dict(dict(dy=fake, s=fake, gamma=fake, mean=fake, rstd=fake, ds_f32=fake, M=8, D=64), **kw))
        return lib.wj_layernorm_pre_bwd(ctypes.byref(a), None)

    assert lib.wj_layernorm_pre_fwd(None, None) == -1 and lib.wj_layernorm_pre_bwd(None, None) == -1
    for bad in (dict(x=None), dict(gamma=None), dict(beta=None), dict(D=66), dict(D=1028), dict(D=0), dict(M=0),
                dict(group_stats=fake, group_rows=0)):
        assert fwd(**bad) == -1, bad
    for bad in (dict(dy=None), dict(s=None), dict(gamma=None), dict(mean=None), dict(rstd=None), dict(D=66), dict(D=2048), dict(M=-3)):
        assert bwd(**bad) == -1, bad
