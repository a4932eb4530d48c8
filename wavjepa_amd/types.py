"""Config dictionaries of the transformer stacks (same keys/defaults as reference wavjepa/types/wavjepa_configs.py:6-63)."""
from __future__ import annotations

from typing import TypedDict

import torch
from torch import nn


class ForwardReturn(TypedDict, total=False):
    local_features: torch.Tensor
    contextual_features: torch.Tensor
    loss: torch.Tensor
    preds: torch.Tensor
    targets: torch.Tensor
    loss_clean: torch.Tensor                # denoiser stage (reference denoiser.py:357-361)
    loss_denoise_dereverb: torch.Tensor


ACTIVATION_KINDS = ("gelu", "relu", "gelu_tanh", "silu")


def activation_kind_of(activation) -> str:
    """The kind of feed-forward activation nn.TransformerEncoderLayer(activation=...) would run, as linear1's GEMM epilogue computes it
    (include/wavjepa_hip_act.h): None / nn.GELU() / "gelu" / F.gelu -> gelu; nn.ReLU() / "relu" / F.relu -> relu;
    nn.GELU(approximate="tanh") / "gelu_tanh" -> gelu_tanh; nn.SiLU() / "silu" / F.silu -> silu.  Anything else is refused here instead
    of being trained as GELU."""
    import torch.nn.functional as F
    a = activation
    if a is None:
        return "gelu"
    if isinstance(a, str):
        if a in ACTIVATION_KINDS:
            return a
    elif type(a) is nn.GELU:
        if a.approximate in ("none", "tanh"):
            return "gelu" if a.approximate == "none" else "gelu_tanh"
    elif type(a) is nn.ReLU:
        return "relu"
    elif type(a) is nn.SiLU:
        return "silu"
    elif a is F.gelu:
        return "gelu"
    elif a is F.relu:
        return "relu"
    elif a is F.silu:
        return "silu"
    what = repr(a) if isinstance(a, str) else (f"{type(a).__name__} ({a!r})" if isinstance(a, nn.Module) else f"{type(a).__name__} {getattr(a, '__name__', a)!r}")
    raise NotImplementedError(f"activation {what}: linear1's GEMM epilogue computes nn.GELU() (gelu), nn.ReLU() (relu), "
                              "nn.GELU(approximate='tanh') (gelu_tanh) and nn.SiLU() (silu)")


class TransformerLayerCFG(TypedDict):
    d_model: int
    nhead: int
    batch_first: bool
    norm_first: bool
    bias: bool
    dim_feedforward: int
    dropout: float
    activation: nn.Module
    layer_norm_eps: float

    @classmethod
    def create(cls, d_model: int = 768, nhead: int = 12, batch_first: bool = True, norm_first: bool = False,
               bias: bool = True, mlp_ratio: float = 4.0, dropout: float = 0.0, activation: nn.Module = None,
               layer_norm_eps: float = 1e-6) -> "TransformerLayerCFG":
        return TransformerLayerCFG(d_model=d_model, nhead=nhead, batch_first=batch_first, norm_first=norm_first, bias=bias,
                                   dim_feedforward=int(d_model * mlp_ratio), dropout=dropout,
                                   activation=activation if activation is not None else nn.GELU(),
                                   layer_norm_eps=layer_norm_eps)


class TransformerEncoderCFG(TypedDict):
    num_layers: int
    enable_nested_tensor: bool
    mask_check: bool

    @classmethod
    def create(cls, num_layers: int = 12, enable_nested_tensor: bool = False, mask_check: bool = True) -> "TransformerEncoderCFG":
        return TransformerEncoderCFG(num_layers=num_layers, enable_nested_tensor=enable_nested_tensor, mask_check=mask_check)
