"""Feed-forward activations on the host: the test helper's fp64 functions against torch's own modules and autograd, the fp32 emulation
of the kernels' formulas inside the helper's bounds over every bf16 input, the mutations the bounds must reject, the module surface
(module -> kind, hyper-parameters, refusals, the launcher's keys) and the C ABI of wj_gemm_bf16_act (struct layout, argument
validation).  The kernels are checked on the GPU (tests/test_activation_ops_gpu.py)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import act_reference as R

SPEC = [(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)]
MODULES = {"relu": nn.ReLU(), "gelu_tanh": nn.GELU(approximate="tanh"), "silu": nn.SiLU()}


# ---------------------------------------------------------------------------------------------------------------- the helper
@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_functions_against_torch_and_autograd(kind):
    g = torch.Generator().manual_seed(3)
    h = (torch.randn(4096, generator=g, dtype=torch.float64) * 3).requires_grad_(True)
    f, f1, f2 = R.act_fns(kind, h.detach())
    y = MODULES[kind](h)
    (d1,) = torch.autograd.grad(y.sum(), h, create_graph=True)
    assert float((y.detach() - f).abs().max()) <= 1e-12
    assert float((d1.detach() - f1).abs().max()) <= 1e-12
    if kind != "relu":
        (d2,) = torch.autograd.grad(d1.sum(), h)
        assert float((d2 - f2).abs().max()) <= 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_is_finite_and_saturates_exactly_on_every_bf16_input(kind):
    v = R.every_bf16()
    v = v[torch.isfinite(v)]
    f, f1, f2 = R.act_fns(kind, v)
    assert bool(torch.isfinite(f).all() and torch.isfinite(f1).all() and torch.isfinite(f2).all())
    big = v >= 64.0
    assert bool((f1[big] == 1.0).all()) and bool((f[big] == v[big].double()).all())
    assert bool((f1[v <= -128.0].float().to(torch.bfloat16) == 0).all())


@pytest.mark.parametrize("kind", ("silu", "gelu_tanh"))
def test_approx_is_four_times_the_measured_emulation_error(kind):
    m = R.measure_approx(kind)
    print(kind, "fp32 emulation against fp64 over every bf16 input:", m, "APPROX", R.APPROX[kind])
    assert 4 * m <= R.APPROX[kind] <= 4 * m * 1.1


@pytest.mark.parametrize("kind", R.KINDS)
def test_emulation_inside_the_bounds_on_every_bf16_input(kind):
    v = R.every_bf16()
    v = v[torch.isfinite(v)]
    g, g1 = R.emulate_f32(kind, v)
    assert bool(torch.isfinite(g).all() and torch.isfinite(g1).all())
    fails, worst = R.check(kind, v.double(), g.to(torch.bfloat16), g1.to(torch.bfloat16))
    assert not fails, fails
    if kind == "relu":
        f, f1, _ = R.act_fns(kind, v)
        assert torch.equal(g.double(), f) and torch.equal(g1.double(), f1)
    big = v >= 64.0
    assert bool((g1[big] == 1.0).all()) and bool((g1[v <= -128.0] == 0).all())


@pytest.mark.parametrize("kind", R.KINDS)
def test_every_mutation_is_rejected(kind):
    g = torch.Generator().manual_seed(5)
    h = (torch.randn(300 * 384, generator=g) * 1.5).to(torch.bfloat16)
    h[::1000] = 0.0                                            # planted h == 0
    h[7::1000] = -3.0
    hd = h.double()
    f, f1, _ = R.act_fns(kind, hd)
    act, act1 = f.float().to(torch.bfloat16), f1.float().to(torch.bfloat16)
    assert not R.check(kind, hd, act, act1)[0]
    names = []
    for name, ma, m1 in R.mutations(kind, hd, act, act1):
        names.append(name)
        assert R.check(kind, hd, ma, m1)[0], f"{kind}: mutation not rejected: {name}"
    assert len(names) >= 2


@pytest.mark.parametrize("kind", ("gelu",) + R.KINDS)
@pytest.mark.parametrize("pre_norm", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_activation_layer_equals_torch_transformer_encoder_layer(kind, pre_norm, masked):
    """The helper's oracle layer against nn.TransformerEncoderLayer(activation=...) in fp32 with the same weights, post- and pre-norm,
    with and without a key-padding mask.  1e-5 relative L2: fp32 round-off of two formulations of one arithmetic."""
    d, h, eps = 64, 4, 1e-6
    module = {"gelu": nn.GELU()}.get(kind) or MODULES[kind]
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=h, dim_feedforward=4 * d, dropout=0.0, activation=module, layer_norm_eps=eps,
                                       batch_first=True, norm_first=pre_norm).train()   # train mode: never the fused inference fast path
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.2 if p.ndim == 2 else 0.1))
            if "norm" in n and n.endswith("weight"):
                p.add_(1.0)
    P = {f"l.{k}": v.detach() for k, v in layer.state_dict().items()}
    x = torch.randn(3, 37, d, generator=torch.Generator().manual_seed(1))
    mask = None
    if masked:
        mask = torch.zeros(3, 37, dtype=torch.bool)
        mask[0, 30:] = True
        mask[2, ::3] = True
    with torch.no_grad():
        want = layer(x, src_key_padding_mask=mask)
        got = R.activation_layer(kind, pre_norm)(P, "l.", x, h, mask, "fp32", eps)
        other = R.activation_layer("relu" if kind != "relu" else "silu", pre_norm)(P, "l.", x, h, mask, "fp32", eps)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())      # noqa: E731
    assert rel(got, want) < 1e-5, rel(got, want)
    assert rel(other, want) > 1e-3                                    # the activation matters at these weights


# ---------------------------------------------------------------------------------------------------------------- module surface
def test_module_to_kind_and_refusals():
    from wavjepa_amd.types import ACTIVATION_KINDS, TransformerLayerCFG, activation_kind_of
    assert ACTIVATION_KINDS == ("gelu", "relu", "gelu_tanh", "silu")
    for a in (None, nn.GELU(), "gelu", F.gelu):
        assert activation_kind_of(a) == "gelu"
    for a in (nn.ReLU(), "relu", F.relu):
        assert activation_kind_of(a) == "relu"
    assert activation_kind_of(nn.GELU(approximate="tanh")) == "gelu_tanh"
    for a in (nn.SiLU(), F.silu):
        assert activation_kind_of(a) == "silu"
    assert activation_kind_of(TransformerLayerCFG.create()["activation"]) == "gelu"
    for bad in (nn.Tanh(), lambda x: x, "swish", nn.LeakyReLU()):
        with pytest.raises(NotImplementedError, match=r"gelu.*relu.*gelu_tanh.*silu") as e:
            activation_kind_of(bad)
        assert ("Tanh" in str(e.value)) == isinstance(bad, nn.Tanh)


def _jepa(act_enc=None, act_dec=None, **kw):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    ext = ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1)
    return JEPA(feature_extractor=ext, transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2, activation=act_enc),
                transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=2),
                transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2, activation=act_dec),
                transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=2), average_top_k_layers=2, **kw)


def test_hyper_parameter_keys_only_when_not_default():
    plain = _jepa()
    assert plain.encoder.activation == plain.decoder.activation == plain.teacher_encoder.activation == "gelu"
    assert not [k for k in plain.hparams if k.startswith("activation")]
    m = _jepa(nn.ReLU(), None)
    assert m.encoder.activation == m.teacher_encoder.activation == "relu" and m.decoder.activation == "gelu"
    assert m.hparams["activation_encoder"] == "relu" and "activation_decoder" not in m.hparams
    assert set(m.hparams) - set(plain.hparams) == {"activation_encoder"}
    m = _jepa(nn.GELU(approximate="tanh"), nn.SiLU())
    assert m.hparams["activation_encoder"] == "gelu_tanh" and m.hparams["activation_decoder"] == "silu"
    with pytest.raises(NotImplementedError, match="Tanh"):
        _jepa(nn.Tanh())


def test_launcher_reads_the_two_keys():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    off, _ = train.build_model(load_config(root, ["trainer.size=tiny"]))
    on, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.activation=relu"]))
    both, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.activation=silu", "trainer.activation_decoder=gelu_tanh"]))
    assert off.encoder.activation == off.decoder.activation == "gelu" and "activation_encoder" not in off.hparams
    assert on.encoder.activation == on.decoder.activation == "relu" and on.hparams["activation_decoder"] == "relu"
    assert both.encoder.activation == "silu" and both.decoder.activation == "gelu_tanh"
    with pytest.raises((ValueError, RuntimeError), match="swish"):
        train.build_model(load_config(root, ["trainer.size=tiny", "trainer.activation=swish"]))


def test_hear_runtime_takes_the_activation():
    from hear_api.runtime import RuntimeJEPA
    from wavjepa_amd.extractors import ConvFeatureExtractor
    ext = lambda: ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1)       # noqa: E731
    rt = RuntimeJEPA(1, None, False, 2.01, ext(), "tiny", 16000, activation=nn.ReLU())
    assert rt.model.encoder.activation == "relu" and rt.model.hparams["activation_encoder"] == "relu"
    assert RuntimeJEPA(1, None, False, 2.01, ext(), "tiny", 16000).model.encoder.activation == "gelu"


def test_denoiser_refuses_another_activation():
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    ext = ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1)
    with pytest.raises(NotImplementedError, match=r"relu.*Denoiser.*gelu"):
        Denoiser(ext, TransformerLayerCFG.create(d_model=64, nhead=2, activation=nn.ReLU()), TransformerEncoderCFG.create(num_layers=1))


def test_engine_refuses_fp8_with_another_activation():
    """The check that lives in engine.py, on a stand-in that has only what it reads (the engine itself needs a GPU)."""
    from wavjepa_amd.engine import EngineConfig, JepaEngine
    fields = {f.name: f.default for f in EngineConfig.__dataclass_fields__.values()}
    assert fields["act_enc"] == "gelu" and fields["act_dec"] == "gelu"
    for kw in (dict(act_enc="relu"), dict(act_dec="silu")):
        cfg = EngineConfig(conv_spec=SPEC, in_channels=1, n_samples=32159, d_enc=64, h_enc=2, l_enc=2, d_dec=64, h_dec=2, l_dec=2, top_k=2, **kw)

        class Stub:
            fp8, recompute = True, False
        s = Stub()
        s.cfg = cfg
        with pytest.raises(RuntimeError, match=r"fp8.*activation"):
            JepaEngine._check_fp8(s)
        s.fp8 = False
        JepaEngine._check_fp8(s)


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_abi_struct_error_codes_and_workspace_query():
    """wj_gemm_bf16_act lives in a library and a header of its own: what libwavjepa_hip.so exports and declares has not moved.  Every
    refusal is answered before any launch, so it can be asked without a GPU (the pointers are never followed)."""
    from wavjepa_amd import _abi, ops
    rel = _abi.load()
    lib = _abi.load("act")
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 and rel.wj_abi_version() == 17
    assert not set(_abi.LIBRARIES["act"].functions) & set(_abi.FUNCTIONS) and "wj_gemm_bf16_act" not in _abi.ENTRY_ARGS
    assert not hasattr(rel, "wj_gemm_bf16_act")
    T, G = _abi.LIBRARIES["act"].struct_types["wj_gemm_act_args"], _abi.STRUCTS["wj_gemm_args"]
    assert ctypes.sizeof(T) == ctypes.sizeof(G) + 8 == lib.wj_act_struct_size(b"wj_gemm_act_args") and T.act.offset == ctypes.sizeof(G)
    assert lib.wj_act_struct_size(b"wj_gemm_args") == -1 and lib.wj_act_struct_size(None) == -1
    assert _abi.LIBRARIES["act"].enums == dict(WJ_ACT_GELU=0, WJ_ACT_RELU=1, WJ_ACT_GELU_TANH=2, WJ_ACT_SILU=3)
    assert ops.ACT == dict(gelu=0, relu=1, gelu_tanh=2, silu=3)

    def args(act=1, **kw):
        f = dict(A=4096, B=8192, C=12288, C2=16384, M=256, N=256, K=128, lda=128, ldb=128, ldc=256, epilogue=ops.EPI_BIAS_GELU2, alpha=1.0)
        f.update(kw)
        return T(gemm=G(**f), act=act)
    rc = lambda a: lib.wj_gemm_bf16_act(ctypes.byref(a), None)                    # noqa: E731
    ARG, UNSUPPORTED = -1, -3
    assert rc(args(act=4)) == ARG and rc(args(act=-1)) == ARG
    for epi in (ops.EPI_BF16, ops.EPI_MUL_GELU_GRAD, ops.EPI_CONV_GELU, ops.EPI_ADD_F32):
        assert rc(args(epilogue=epi)) == ARG
    assert rc(args(C2=0)) == ARG and rc(args(A=0)) == ARG and rc(args(N=260)) == ARG and rc(args(schedule=8)) == ARG
    assert rc(args(schedule=6)) == UNSUPPORTED and rc(args(schedule=7)) == UNSUPPORTED
    assert rc(args(schedule=2)) == UNSUPPORTED and rc(args(b_trans=1)) == UNSUPPORTED
    assert lib.wj_gemm_bf16_act(None, None) == ARG
    assert _abi.workspace_bytes("wj_gemm_bf16_act", args()) == 0
    assert lib.wj_act_workspace_bytes(b"wj_gemm_bf16", ctypes.byref(args())) == -1
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", _abi.LIBRARIES["act"].path], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1] for ln in syms.splitlines() if " T " in ln)
    assert exported == ["wj_act_struct_size", "wj_act_workspace_bytes", "wj_gemm_bf16_act"], exported
