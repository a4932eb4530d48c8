"""Conv stack of mode="layer_norm" for the oracle.  TEST INFRASTRUCTURE ONLY (a helper, not a test).

`oracle/jepa_oracle.py` knows the default front-end only (GroupNorm on layer 0); its `conv_frontend` looks `_conv_stack` up as a
module global on every call.  `conv_stack_layer_norm` below is written from the oracle's own conventions -- parameters by
state-dict name, [N, C_in, L] in, [N, T, C] out, "fp32" / "bf16" dtype flows -- so

    monkeypatch.setattr(J, "_conv_stack", conv_stack_layer_norm)

turns the whole oracle (jepa_forward, its autograd gradients, audio_representation, train_step) into the oracle of this mode, for
`cnn.` and `cnns.{c}.` stacks.  Layer l: Conv1d(+ bias when `{stack}{l}.0.bias` exists) -> LayerNorm over channels
(`{stack}{l}.2.1.{weight,bias}`, eps 1e-5) -> erf-GELU.
bf16 mode: conv operands and output bf16 (autocast), LayerNorm and GELU in fp32 (autocast's fp32 policy for layer_norm; GELU keeps
its input dtype), the layer output rounded to bf16 -- the next conv's operand, and after the last layer the point where the HIP
path rounds while stock autocast hands feature_norms the fp32 tensor (PARITY.md).
tests/test_conv_layernorm_cpu.py pins the fp32 flow to the reference's extractor classes (tests/golden/conv_layernorm.npz).
"""
import torch
import torch.nn.functional as F


def conv_stack_layer_norm(P, x: torch.Tensor, spec, mode: str, stack: str) -> torch.Tensor:
    for i, (dim, k, s) in enumerate(spec):
        w, b = P[f"{stack}{i}.0.weight"], P.get(f"{stack}{i}.0.bias")
        if mode == "bf16":
            x = F.conv1d(x.to(torch.bfloat16), w.to(torch.bfloat16), None if b is None else b.to(torch.bfloat16), stride=s)
        else:
            x = F.conv1d(x.float(), w.float(), None if b is None else b.float(), stride=s)
        g, be = P[f"{stack}{i}.2.1.weight"], P[f"{stack}{i}.2.1.bias"]
        z = F.layer_norm(x.float().transpose(1, 2), (dim,), g.float(), be.float(), 1e-5)
        x = F.gelu(z).transpose(1, 2)
        if mode == "bf16":
            x = x.to(torch.bfloat16)
    return x.transpose(1, 2)
