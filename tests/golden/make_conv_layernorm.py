"""Generates tests/golden/conv_layernorm.npz from the reference's extractor classes in mode="layer_norm" (test tooling; runs ONLY
where the read-only reference is present, through _ref_import.install_stubs()).

CPU, fp32, a small spec (C = 16, 4 layers, 2 clips of 800 samples): the mono stack (ConvFeatureExtractor) and a 2-channel
own-weights stack (ConvChannelFeatureExtractor), each with conv_bias True and False.  Per case the file holds the synthetic weights
under their state-dict names (`<case>.w.<name>`), the input (`<case>.x`), the output (`<case>.y`) and every parameter's gradient of
output.square().sum() (`<case>.g.<name>`).

    python tests/golden/make_conv_layernorm.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import  # noqa: E402
import synth  # noqa: E402

SPEC = [(16, 10, 5), (16, 3, 2), (16, 3, 2), (16, 2, 2)]
N_CLIPS, N_SAMPLES = 2, 800


def synth_weight(name, shape, seed=11):
    """Conv weights and biases by synth's rules; LayerNorm gains around 1 (synth.synth_tensor knows the GroupNorm name only)."""
    if name.endswith(".2.1.weight"):
        return (1.0 + 0.1 * synth.hash_uniform(int(np.prod(shape)), synth.name_seed(name, seed))).reshape(shape).astype(np.float32)
    return synth.synth_tensor(name, shape, seed)


def main():
    _ref_import.install_stubs()
    from wavjepa.extractors.audio_channel_feature_extractor import ConvChannelFeatureExtractor
    from wavjepa.extractors.audio_feature_extractor import ConvFeatureExtractor
    out = {}
    for kind, cls, chans, extra in (("mono", ConvFeatureExtractor, 1, {}),
                                    ("chan", ConvChannelFeatureExtractor, 2, dict(share_weights_over_channels=False))):
        for bias in (True, False):
            case = f"{kind}_{'bias' if bias else 'nobias'}"
            torch.manual_seed(0)
            ext = cls(conv_layers_spec=SPEC, in_channels=chans, dropout=0.0, mode="layer_norm", conv_bias=bias, depthwise=False, **extra)
            ext = ext.float().train()
            sd = {k: torch.from_numpy(synth_weight(k, tuple(v.shape))) for k, v in ext.state_dict().items()}
            ext.load_state_dict(sd)
            x = torch.from_numpy(synth.synth_audio(N_CLIPS, chans, N_SAMPLES, seed=5))
            y = ext(x)
            y.square().sum().backward()
            out[f"{case}.x"] = x.numpy()
            out[f"{case}.y"] = y.detach().numpy()
            for k, p in ext.named_parameters():
                out[f"{case}.w.{k}"] = p.detach().numpy()
                out[f"{case}.g.{k}"] = p.grad.numpy()
            print(case, tuple(y.shape), len(sd), "tensors")
    path = os.path.join(HERE, "conv_layernorm.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
