"""Pre-norm (norm_first=True) transformer layer for the oracle.  TEST INFRASTRUCTURE ONLY (a helper, not a test).

`oracle/jepa_oracle.py` knows the post-norm layer only; its `encoder_stack` looks `post_norm_layer` up as a module global on
every call.  `pre_norm_layer` below is written from the oracle's own `_lin`, `attention` and `_ln` -- the same dtype flow, the
residual stream fp32, every Linear operand bf16 in "bf16" mode -- so

    monkeypatch.setattr(J, "post_norm_layer", pre_norm_layer)

turns the whole oracle (jepa_forward, its autograd gradients, audio_representation, train_step) into a pre-norm oracle for the
student, the teacher and the predictor.  `mixed_layer(prefixes)` switches by the layer's parameter prefix, for models where only
some stacks are pre-norm.  tests/test_prenorm_cpu.py pins `pre_norm_layer` to torch.nn.TransformerEncoderLayer(norm_first=True).
"""
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F

from oracle import jepa_oracle as J

_POST_NORM_LAYER = J.post_norm_layer          # the oracle's own layer, whatever a test patches into the module later


def pre_norm_layer(P, pre: str, x: torch.Tensor, nhead: int, key_mask: Optional[torch.Tensor], mode: str,
                   eps: float = 1e-6) -> torch.Tensor:
    """x = x + out_proj(attn(in_proj(LN1(x))));  x = x + linear2(gelu(linear1(LN2(x)))).  x is fp32."""
    y = J._ln(x, P[pre + "norm1.weight"], P[pre + "norm1.bias"], eps)
    qkv = J._lin(y, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"], mode)
    a = J.attention(qkv, nhead, key_mask, mode)
    sa = J._lin(a, P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"], mode)
    x = x.float() + sa.float()
    y = J._ln(x, P[pre + "norm2.weight"], P[pre + "norm2.bias"], eps)
    h = J._lin(y, P[pre + "linear1.weight"], P[pre + "linear1.bias"], mode)
    h = F.gelu(h)
    ff = J._lin(h, P[pre + "linear2.weight"], P[pre + "linear2.bias"], mode)
    return x + ff.float()


def mixed_layer(pre_norm_prefixes: Sequence[str]) -> Callable:
    """A layer function for J.post_norm_layer's place: pre-norm for layers whose parameter prefix starts with one of
    `pre_norm_prefixes` ("encoder.", "teacher_encoder.", "decoder."), the oracle's post-norm layer for the others."""
    prefixes = tuple(pre_norm_prefixes)

    def layer(P, pre, x, nhead, key_mask, mode, eps=1e-6):
        fn = pre_norm_layer if pre.startswith(prefixes) else _POST_NORM_LAYER
        return fn(P, pre, x, nhead, key_mask, mode, eps)
    return layer


STUDENT_TEACHER = ("encoder.", "teacher_encoder.")     # the student and its EMA teacher share one layout
PREDICTOR = ("decoder.",)
