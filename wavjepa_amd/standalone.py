"""Stand-alone use of the conv front-end kernels (ConvFeatureExtractor.forward outside a JEPA module)."""
from __future__ import annotations

import torch

from . import ops
from .conv_frontend import ConvFrontend, ConvLayerParams


def _layer_params(layer, l: int, dev) -> ConvLayerParams:
    """One Sequential(conv, dropout, norm..., GELU) of an extractor's stack: the conv weight as bf16 (layer 0) or fp32 (the GEMM
    layouts' source), the other parameters fp32."""
    f32 = lambda t: None if t is None else t.detach().to(dev, torch.float32).contiguous()
    conv, norm = layer[0], layer[2]
    w = conv.weight.detach().to(dev, torch.bfloat16).contiguous() if l == 0 else f32(conv.weight)
    if isinstance(norm, torch.nn.Sequential):             # mode="layer_norm": Sequential(-, LayerNorm, -) behind every conv
        ln = norm[1]
        return ConvLayerParams(w, f32(conv.bias), f32(ln.weight), f32(ln.bias), eps=ln.eps)
    if l == 0:                                            # mode="default": GroupNorm behind conv 0 only
        return ConvLayerParams(w, None, f32(norm.weight), f32(norm.bias))
    return ConvLayerParams(w)


@torch.no_grad()
def conv_frontend_tokens(extractor, x: torch.Tensor) -> torch.Tensor:
    """x [N, C_in, L] on the GPU -> tokens bf16 (the front-end's forward: the layer-0 kernel, then one implicit GEMM per layer).
    ConvFeatureExtractor: [N, T, C].  ConvChannelFeatureExtractor: every channel through its mono stack, flattened channel-major
    [N, C_in * T, C] (reference audio_channel_feature_extractor.py:154-179)."""
    ops.require_gpu()
    if not x.is_cuda:
        raise RuntimeError("the conv front-end needs GPU tensors (no CPU fallback)")
    audio = x.to(torch.bfloat16).contiguous()
    N, C_in, n_samples = audio.shape
    if hasattr(extractor, "cnns"):
        streams, stacks = C_in, [extractor.cnns[0]] if extractor.weight_sharing else list(extractor.cnns)[:C_in]
    else:
        streams, stacks = 1, [extractor.cnn]
    params = [[_layer_params(layer, l, audio.device) for l, layer in enumerate(cnn)] for cnn in stacks]
    front = ConvFrontend(extractor.conv_layers_spec, C_in // streams, n_samples, streams, params, isinstance(stacks[0][0][2], torch.nn.Sequential),
                         audio.device, backward=False)
    front.alloc(N, train=False)
    front.forward(audio)
    out = front.tokens()
    torch.cuda.current_stream().synchronize()   # the front-end's buffers and the converted parameters must outlive the kernels
    return out
