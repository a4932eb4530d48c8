"""Dropout on the host: the generator's known answers, the test helper's layer against torch's own nn.TransformerEncoderLayer(dropout=p)
with the helper's masks, the module surface (construction, hyper-parameters, refusals, the launcher's keys) and the C ABI of the five
new entries (struct layout, argument validation).  The kernels are checked on the GPU (tests/test_dropout_ops_gpu.py,
tests/test_dropout_gpu.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

from oracle import jepa_oracle as J
from tests import dropout_reference as R

SPEC = [(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)]


# ---------------------------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(w) for w in R.philox4x32_10(*ctr, *key))
    assert got == want, [hex(g) for g in got]


def test_threshold_and_scale():
    assert R.thr_scale(0.1)[0] == 6554 and R.thr_scale(0.5)[0] == 32768 and R.thr_scale(1 / 65536)[0] == 1
    assert R.thr_scale(0.0)[0] == 0 and float(R.thr_scale(0.0)[1]) == 1.0
    assert R.thr_scale(0.5)[1] == np.float32(2.0) and R.thr_scale(0.1)[1].dtype == np.float32


def test_masks_depend_on_every_counter_field_and_hit_the_rate():
    base = R.row_keep(7, 3, 0, 1, R.SITE_RES1, 67, 384, 0.1)
    for other in (R.row_keep(8, 3, 0, 1, R.SITE_RES1, 67, 384, 0.1), R.row_keep(7, 4, 0, 1, R.SITE_RES1, 67, 384, 0.1),
                  R.row_keep(7, 3, 1, 1, R.SITE_RES1, 67, 384, 0.1), R.row_keep(7, 3, 0, 2, R.SITE_RES1, 67, 384, 0.1),
                  R.row_keep(7, 3, 0, 1, R.SITE_RES2, 67, 384, 0.1), R.row_keep(7 + (1 << 32), 3, 0, 1, R.SITE_RES1, 67, 384, 0.1)):
        assert 0.1 < float((base != other).mean()) < 0.3          # two independent masks at p = 0.1 differ on ~18 % of the elements
    big = R.row_keep(1, 0, 0, 0, R.SITE_FFN, 400, 3072, 0.1)
    pe = 6554 / 65536
    assert abs(big.mean() - (1 - pe)) < 5 * np.sqrt(pe * (1 - pe) / big.size)
    a = R.attn_keep(7, 3, 1, 0, 3, 2, 129, 129, 0.1)
    assert a.shape == (3, 2, 129, 129) and not np.array_equal(a[0, 0], a[0, 1]) and not np.array_equal(a[0, 0], a[0, 0].T)
    assert np.array_equal(a[:, :, :17, :17], R.attn_keep(7, 3, 1, 0, 3, 2, 17, 17, 0.1))      # the mask of (b, h, q, k) does not depend on T
    assert abs(a.mean() - (1 - pe)) < 5 * np.sqrt(pe * (1 - pe) / a.size)


# ---------------------------------------------------------------------------------------------------------------- the helper's layer
def _torch_layer(d, h, p, eps):
    layer = nn.TransformerEncoderLayer(d_model=d, nhead=h, dim_feedforward=4 * d, dropout=p, activation="gelu", layer_norm_eps=eps,
                                       batch_first=True, norm_first=False).double()
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, q in layer.named_parameters():
            q.copy_(torch.randn(q.shape, generator=g, dtype=torch.float64) * (0.2 if q.ndim == 2 else 0.1))
            if "norm" in n and n.endswith("weight"):
                q.add_(1.0)
    return layer.train()


def rel(a, b):
    return float((a.detach().double() - b.detach().double()).norm() / (b.detach().double().norm() + 1e-300))


@pytest.mark.parametrize("masked", [False, True])
def test_helper_layer_equals_torch_layer_with_the_same_masks(monkeypatch, masked):
    """nn.TransformerEncoderLayer(dropout=p) in fp64 train mode, torch.nn.functional.dropout replaced by a function that hands out the
    helper's masks in call order (attention probabilities, dropout1, FFN dropout, dropout2), _sa_block routed through
    need_weights=True so that the probabilities pass through it: forward and input gradient to 1e-12 relative."""
    d, h, p, eps, B, T = 64, 2, 0.1, 1e-6, 3, 37
    layer = _torch_layer(d, h, p, eps)
    P = {f"l.{k}": v.detach() for k, v in layer.state_dict().items()}
    sc = float(R.thr_scale(p)[1])
    m = dict(attn=torch.from_numpy(R.attn_keep(11, 2, 0, 0, B, h, T, T, p)).double() * sc,
             res1=torch.from_numpy(R.row_keep(11, 2, 0, 0, R.SITE_RES1, B * T, d, p)).reshape(B, T, d).double() * sc,
             ffn=torch.from_numpy(R.row_keep(11, 2, 0, 0, R.SITE_FFN, B * T, 4 * d, p)).reshape(B, T, 4 * d).double() * sc,
             res2=torch.from_numpy(R.row_keep(11, 2, 0, 0, R.SITE_RES2, B * T, d, p)).reshape(B, T, d).double() * sc)
    queue = [m["attn"], m["res1"], m["ffn"], m["res2"]]

    def handed_out(x, p=0.5, training=True, inplace=False):
        assert training
        return x * queue.pop(0).reshape(x.shape)
    monkeypatch.setattr(torch.nn.functional, "dropout", handed_out)

    def sa_block(x, attn_mask, key_padding_mask, is_causal=False):
        y = layer.self_attn(x, x, x, attn_mask=attn_mask, key_padding_mask=key_padding_mask, need_weights=True)[0]
        return layer.dropout1(y)
    monkeypatch.setattr(layer, "_sa_block", sa_block)
    mask = None
    if masked:
        mask = torch.zeros(B, T, dtype=torch.bool)
        mask[0, 30:] = True
        mask[2, ::3] = True
    x = torch.randn(B, T, d, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    want = layer(xa, src_key_padding_mask=mask)
    assert not queue
    got = R.dropout_layer(P, "l.", xb, h, mask, "fp64", eps, m)
    w = torch.randn(want.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (want * w).sum().backward()
    (got * w).sum().backward()
    assert rel(got, want) < 1e-12 and rel(xb.grad, xa.grad) < 1e-12, (rel(got, want), rel(xb.grad, xa.grad))
    plain = R.dropout_layer(P, "l.", x, h, mask, "fp64", eps, None)
    assert rel(plain, want) > 1e-2                   # (the masks matter)


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_helper_layer_without_masks_is_the_oracles_layer(mode):
    d, h = 64, 2
    P = {f"l.{k}": v.detach().float() for k, v in _torch_layer(d, h, 0.0, 1e-6).state_dict().items()}
    x = torch.randn(2, 19, d, generator=torch.Generator().manual_seed(3))
    mask = torch.zeros(2, 19, dtype=torch.bool)
    mask[1, 15:] = True
    assert torch.equal(R.dropout_layer(P, "l.", x, h, mask, mode), J.post_norm_layer(P, "l.", x, h, mask, mode))


# ---------------------------------------------------------------------------------------------------------------- module surface
def _jepa(p_enc=0.0, p_dec=0.0, **kw):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    enc = dict(d_model=64, nhead=2, dropout=p_enc)
    enc.update(kw.pop("enc", {}))
    dec = dict(d_model=64, nhead=2, dropout=p_dec)
    dec.update(kw.pop("dec", {}))
    return JEPA(feature_extractor=ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1),
                transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=2),
                transformer_encoder_layers_cfg=TransformerLayerCFG.create(**enc),
                transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=2),
                transformer_decoder_layers_cfg=TransformerLayerCFG.create(**dec),
                average_top_k_layers=2, process_audio_seconds=2.01, nr_samples_per_audio=2, **kw)


def test_jepa_with_dropout_constructs_on_a_cpu_only_host():
    torch.manual_seed(1234)
    m = _jepa(0.1, 0.1)
    assert m.encoder.dropout == 0.1 and m.decoder.dropout == 0.1 and m.teacher_encoder.dropout == 0.1   # (the engine never drops in the teacher)
    assert m.dropout_seed == 1234 and m.dropout_call is None
    assert m.hparams["dropout_encoder"] == 0.1 and m.hparams["dropout_decoder"] == 0.1 and m.hparams["dropout_seed"] == 1234
    only_enc = _jepa(0.2, 0.0)
    assert only_enc.hparams["dropout_encoder"] == 0.2 and only_enc.hparams["dropout_decoder"] == 0.0
    assert list(m.state_dict()) == list(_jepa().state_dict())


def test_default_models_hyper_parameters_are_the_set_they_were():
    from tests.test_recompute_cpu import DEFAULT_HPARAMS, plain_path
    m = _jepa()
    assert not {"dropout_encoder", "dropout_decoder", "dropout_seed"} & set(m.hparams)
    if plain_path():
        assert set(m.hparams) == DEFAULT_HPARAMS
    assert m.encoder.dropout == 0.0 and m.decoder.dropout == 0.0


def test_refused_combinations_name_both_options():
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    with pytest.raises(NotImplementedError, match=r"dropout.*norm_first"):
        _jepa(0.1, 0.0, enc=dict(norm_first=True))
    with pytest.raises(NotImplementedError, match=r"dropout.*norm_first"):
        _jepa(0.0, 0.1, dec=dict(norm_first=True))
    with pytest.raises(NotImplementedError, match=r"dropout.*16-wide heads"):
        _jepa(0.0, 0.1, dec=dict(d_model=64, nhead=4))
    with pytest.raises(NotImplementedError, match=r"dropout.*16-wide heads"):
        _jepa(0.0, 0.1, size="tiny")                 # the tiny predictor: 4 heads of 16
    assert _jepa(0.1, 0.0, size="tiny").encoder.dropout == 0.1      # (its student has 32-wide heads)
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError, match=r"dropout.*\[0, 1\)"):
            _jepa(bad, 0.0)
    with pytest.raises(NotImplementedError, match=r"dropout.*Denoiser"):
        Denoiser(ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1), TransformerLayerCFG.create(d_model=64, nhead=2, dropout=0.1),
                 TransformerEncoderCFG.create(num_layers=1))
    with pytest.raises(NotImplementedError, match="dropout"):
        ConvFeatureExtractor(conv_layers_spec=SPEC, in_channels=1, dropout=0.1)


def test_engine_refuses_fp8_with_dropout_and_checks_its_config():
    """The checks that live in engine.py, on a stand-in that has only what they read (the engine itself needs a GPU)."""
    from wavjepa_amd.engine import EngineConfig, JepaEngine
    fields = {f.name: f.default for f in EngineConfig.__dataclass_fields__.values()}
    assert fields["dropout_enc"] == 0.0 and fields["dropout_dec"] == 0.0
    cfg = EngineConfig(conv_spec=SPEC, in_channels=1, n_samples=32159, d_enc=64, h_enc=2, l_enc=2, d_dec=64, h_dec=2, l_dec=2, top_k=2,
                       dropout_enc=0.1)

    class Stub:
        fp8, recompute = True, False
    s = Stub()
    s.cfg = cfg
    with pytest.raises(RuntimeError, match=r"fp8.*dropout"):
        JepaEngine._check_fp8(s)
    s.fp8 = False
    JepaEngine._check_fp8(s)


def test_launcher_reads_the_two_keys():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    off, _ = train.build_model(load_config(root, ["trainer.size=tiny"]))
    on, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.dropout_encoder=0.1"]))
    both, _ = train.build_model(load_config(root, ["trainer.dropout_encoder=0.1", "trainer.dropout_decoder=0.05"]))
    assert off.encoder.dropout == 0.0 and off.decoder.dropout == 0.0 and "dropout_encoder" not in off.hparams
    assert on.encoder.dropout == 0.1 and on.decoder.dropout == 0.0
    assert both.encoder.dropout == 0.1 and both.decoder.dropout == 0.05


# ---------------------------------------------------------------------------------------------------------------- C ABI
NEW = dict(wj_dropout_rows="wj_dropout_rows_args", wj_layernorm_fwd_drop="wj_ln_fwd_drop_args", wj_layernorm_bwd_drop="wj_ln_bwd_drop_args",
           wj_attn_stream_fwd_drop="wj_attn_fwd_drop_args", wj_attn_stream_bwd_drop="wj_attn_bwd_drop_args")


def test_abi_version_is_still_17_and_the_new_structs_append_the_tail():
    """The dropout entries live in a library and a header of their own: what libwavjepa_hip.so exports and declares has not moved."""
    import subprocess
    from wavjepa_amd import _abi
    rel = _abi.load()
    lib = _abi.load("dropout")
    S = {**_abi.STRUCTS, **_abi.LIBRARIES["dropout"].struct_types}
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 and rel.wj_abi_version() == 17
    assert not set(_abi.LIBRARIES["dropout"].functions) & set(_abi.FUNCTIONS) and not set(NEW) & set(_abi.ENTRY_ARGS)
    assert not any(hasattr(rel, fn) for fn in NEW)
    assert ctypes.sizeof(S["wj_dropout_args"]) == 24 == lib.wj_dropout_struct_size(b"wj_dropout_args")
    assert ctypes.sizeof(S["wj_dropout_rows_args"]) == 56
    assert lib.wj_dropout_struct_size(b"wj_no_such_struct") == -1 and lib.wj_dropout_struct_size(None) == -1
    for fn, name in NEW.items():
        assert fn in _abi.LIBRARIES["dropout"].functions and hasattr(lib, fn) and _abi.LIBRARIES["dropout"].entry_args[fn] == name
        assert lib.wj_dropout_struct_size(name.encode()) == ctypes.sizeof(S[name]) > 0
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIBRARIES["dropout"].path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert exported == set(_abi.LIBRARIES["dropout"].functions) == set(NEW) | {"wj_dropout_struct_size", "wj_dropout_workspace_bytes"}, sorted(exported)
    for name, parent in (("wj_ln_fwd_drop_args", "wj_ln_fwd_args"), ("wj_ln_bwd_drop_args", "wj_ln_bwd_args"),
                         ("wj_attn_fwd_drop_args", "wj_attn_fwd_args"), ("wj_attn_bwd_drop_args", "wj_attn_bwd_args")):
        assert ctypes.sizeof(S[name]) == ctypes.sizeof(S[parent]) + 24      # the parent's struct, then the tail
    assert (ctypes.sizeof(S["wj_ln_fwd_args"]), ctypes.sizeof(S["wj_ln_bwd_args"]), ctypes.sizeof(S["wj_attn_fwd_args"]),
            ctypes.sizeof(S["wj_attn_bwd_args"])) == (136, 144, 64, 104)     # ... which have not moved


def _call(fn, a):
    from wavjepa_amd import _abi
    return int(getattr(_abi.load("dropout"), fn)(ctypes.byref(a), None))


def test_argument_errors_are_answered_before_a_launch():
    from wavjepa_amd import _abi, ops
    S = {**_abi.STRUCTS, **_abi.LIBRARIES["dropout"].struct_types}
    lib = _abi.load("dropout")
    for fn in NEW:
        assert int(getattr(lib, fn)(None, None)) == -1
    ptr = 4096                                            # never dereferenced: every call below is refused on the host
    good = ops.drop_args(1, 0, 0.1, site=2)
    rows = lambda **kw: S["wj_dropout_rows_args"](**dict(dict(x=ptr, ldx=64, M=4, N=64, drop=good), **kw))
    assert _call("wj_dropout_rows", rows(x=0)) == -1
    assert _call("wj_dropout_rows", rows(N=60, ldx=60)) == -1
    assert _call("wj_dropout_rows", rows(ldx=68)) == -1
    assert _call("wj_dropout_rows", rows(M=0)) == -1
    for p in (-0.1, 1.0, 2.0, float("nan")):
        assert _call("wj_dropout_rows", rows(drop=ops.drop_args(1, 0, p, site=3))) == -1
    ln = lambda **kw: S["wj_ln_fwd_args"](**dict(dict(x=ptr, r=ptr, gamma=ptr, beta=ptr, y_f32=ptr, M=4, D=64, eps=1e-6), **kw))
    fwd = lambda l, d=good: S["wj_ln_fwd_drop_args"](ln=l, drop=d)
    assert _call("wj_layernorm_fwd_drop", fwd(ln(x=0))) == -1
    assert _call("wj_layernorm_fwd_drop", fwd(ln(r=0))) == -1                 # the addend is what is dropped
    assert _call("wj_layernorm_fwd_drop", fwd(ln(D=60))) == -1                # D % 8
    assert _call("wj_layernorm_fwd_drop", fwd(ln(D=2048))) == -1
    assert _call("wj_layernorm_fwd_drop", fwd(ln(), ops.drop_args(1, 0, 1.0, site=2))) == -1
    lb = lambda **kw: S["wj_ln_bwd_args"](**dict(dict(dy=ptr, x=ptr, r=ptr, gamma=ptr, mean=ptr, rstd=ptr, ds_f32=ptr, M=4, D=64), **kw))
    bwd = lambda l, d=good: S["wj_ln_bwd_drop_args"](ln=l, drop=d)
    assert _call("wj_layernorm_bwd_drop", bwd(lb(dy=0))) == -1
    assert _call("wj_layernorm_bwd_drop", bwd(lb(r=0))) == -1
    assert _call("wj_layernorm_bwd_drop", bwd(lb(D=60))) == -1
    assert _call("wj_layernorm_bwd_drop", bwd(lb(), ops.drop_args(1, 0, -0.5, site=2))) == -1
    af = lambda **kw: S["wj_attn_fwd_args"](**dict(dict(qkv=ptr, out=ptr, B=2, T=64, H=2, hd=32, mask_group=1), **kw))
    afd = lambda a, d=good: S["wj_attn_fwd_drop_args"](attn=a, drop=d)
    assert _call("wj_attn_stream_fwd_drop", afd(af(qkv=0))) == -1
    assert _call("wj_attn_stream_fwd_drop", afd(af(T=1025))) == -1
    assert _call("wj_attn_stream_fwd_drop", afd(af(hd=16))) == -3
    assert _call("wj_attn_stream_fwd_drop", afd(af(), ops.drop_args(1, 0, 1.0, site=1))) == -1
    ab = lambda **kw: S["wj_attn_bwd_args"](**dict(dict(qkv=ptr, out=ptr, dout=ptr, lse=ptr, dqkv=ptr, B=2, T=64, H=2, hd=32, mask_group=1), **kw))
    abd = lambda a, d=good: S["wj_attn_bwd_drop_args"](attn=a, drop=d)
    assert _call("wj_attn_stream_bwd_drop", abd(ab(lse=0))) == -1
    assert _call("wj_attn_stream_bwd_drop", abd(ab(hd=16))) == -3
    assert _call("wj_attn_stream_bwd_drop", abd(ab(dbias=ptr))) == -1          # dbias without dbias_ws
    assert _call("wj_attn_stream_bwd_drop", abd(ab(), ops.drop_args(1, 0, 1.5, site=1))) == -1
    assert ops.workspace_bytes("wj_layernorm_bwd_drop", ln=S["wj_ln_bwd_args"](D=768)) == ops.workspace_bytes("wj_layernorm_bwd", D=768)
    assert ops.workspace_bytes("wj_attn_stream_bwd_drop", attn=S["wj_attn_bwd_args"](B=8, H=2, hd=64)) == 8 * 3 * 128 * 4
    assert int(lib.wj_dropout_workspace_bytes(b"wj_no_such_entry", ctypes.byref(S["wj_dropout_args"]()))) == -1
    for fn, name in NEW.items():                       # a zeroed struct of every entry is answered in-process
        assert int(lib.wj_dropout_workspace_bytes(fn.encode(), ctypes.byref(S[name]()))) >= 0, fn


def test_dropout_library_kernels_have_no_mfma_result_read_across_a_branch(tmp_path):
    """tools/mfma_hazard_scan.py over the gfx950 assembly of the dropout library's sources, compiled as that library compiles them
    (tests/test_host_cpu.py scans the release library's)."""
    import subprocess
    import sys
    from concurrent.futures import ThreadPoolExecutor
    from wavjepa_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = B._hipcc()

    def scan(src):
        asm = str(tmp_path / (src + ".s"))
        r = subprocess.run([hipcc] + [f for f in B.FLAGS if f != "-fPIC"] + B.LIBRARIES["dropout"].flags + ["-S", "--cuda-device-only", "-o", asm,
                            os.path.join(root, "wavjepa_amd", "csrc", src)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([sys.executable, os.path.join(root, "tools", "mfma_hazard_scan.py"), asm], capture_output=True, text=True)
        return src, r.returncode, r.stdout[-1500:]
    with ThreadPoolExecutor(max_workers=4) as ex:
        for src, rc, out in ex.map(scan, B.LIBRARIES["dropout"].sources):
            assert rc == 0, (src, out)
