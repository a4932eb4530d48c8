"""The masked-loss family (mse, l1, smooth_l1, huber) on the host: tests/loss_reference.py against torch.nn's losses in float64, its
fp32 emulation against its bounds, the mutations the bounds must reject, the C ABI of wj_masked_loss and the module surface
(JEPA's loss_fn mapping, hparams).  Worst emulation error / bound over all cases: see PARITY.md.
"""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import loss_reference as lr
from tests import norm_reference as nr

CASES = [(1, 1, 1, 4), (2, 3, 37, 384), (3, 4, 50, 768), (2, 2, 33, 1000)]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def ragged_rows(c, n):
    """the targets and every third of the other rows, in dense order (the rule of test_masked_mse)"""
    keep = (c["tgt"] != 0) | (torch.arange(n) % 3 == 0)
    return torch.nonzero(keep).squeeze(1).to(torch.int32)


def variants(B, G, T, D, beta):
    """(tag, case, keyword arguments): the variants of the GPU test that reach the arithmetic"""
    c = lr.plant(nr.mse_inputs(B, G, T, D, 700), B, G, T, D, beta)
    rows = ragged_rows(c, B * G * T)
    yield "mixed", c, {}
    yield "zeros", lr.plant(nr.mse_inputs(B, G, T, D, 701, "zeros"), B, G, T, D, beta), {}
    yield "ones", lr.plant(nr.mse_inputs(B, G, T, D, 702, "ones"), B, G, T, D, beta), {}
    yield "gscale", c, dict(gscale=0.5, gscale_dev=3.0)
    yield "ragged", dict(c, preds=c["preds"][rows.long()]), dict(rows=rows)


# ------------------------------------------------------------------------------------------------------------ torch float64
@pytest.mark.parametrize("kind,beta", lr.GRID)
def test_reference_equals_torch_losses_in_float64(kind, beta):
    """the reference's masked_loss (loss_fn(pred, target) per element, mean over D, masked sum / (count + 1e-8)) with torch.nn's module
    in float64, and its autograd gradient"""
    B, G, T, D = 2, 3, 5, 8
    c = lr.plant(nr.mse_inputs(B, G, T, D, 4), B, G, T, D, beta)
    pr = c["preds"].double().requires_grad_(True)
    mask = (c["tgt"].reshape(B, G, T) != 0)
    tg = c["targets"].double()[:, None].expand(B, G, T, D)
    per = lr.torch_loss_module(kind, beta)(pr.view(B, G, T, D), tg).mean(-1) * mask
    loss = per.sum() / (mask.sum().double() + nr.f32eps(1e-8))
    loss.backward()
    ref = lr.masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta)
    assert rel(ref["loss"][0][0], loss.detach()) < 1e-12 and float(ref["loss"][0][1]) == float(mask.sum())
    if kind == "mse":
        assert rel(ref["dpreds"][0], nr.bf16(pr.grad)) < 1e-12
    else:
        assert rel(ref["_v"][0], pr.grad) < 1e-12
        r, _, _ = c["planted"]
        assert float(ref["_v"][0][r, 0]) == 0.0 == float(pr.grad[r, 0])          # sign(0) = 0, in torch too
    # the oracle-side objective is the same expression in fp32
    o = lr.oracle_masked_loss(kind, beta)(c["preds"].reshape(B * G, T, D), c["targets"], mask)
    assert abs(float(o) - float(loss.detach())) < 1e-5 * abs(float(loss.detach()))


def test_branch_shares_of_the_kernel_cases():
    """a condition of the cases, not a measurement: wherever a case has >= 1000 target elements, at least 10 % of them lie on each side
    of the branch, for every beta of the tests"""
    for B, G, T, D in CASES:
        for beta in lr.BETAS:
            c = lr.plant(nr.mse_inputs(B, G, T, D, 700), B, G, T, D, beta)
            n, share = lr.quadratic_share(c, B, G, T, D, beta)
            print(f"B,G,T,D={B, G, T, D} beta={beta}: {n} target elements, {share:.3f} with |d| < beta")
            if n >= 1000:
                assert 0.1 <= share <= 0.9, (B, G, T, D, beta, share)


# ------------------------------------------------------------------------------------------------------------ emulation, mutations
def test_emulation_stays_inside_every_bound():
    worst = {}
    for B, G, T, D in CASES:
        for kind, beta in lr.GRID:
            for tag, c, kw in variants(B, G, T, D, beta):
                got = lr.emulate_masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, **kw)
                ref = lr.masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, **kw)
                for k in ("loss", "dpreds"):
                    w = nr.check(t(got[k]), *ref[k], what=f"{kind} beta={beta} {B, G, T, D} {tag} {k}")
                    worst[(kind, k)] = max(worst.get((kind, k), 0.0), w)
    print()
    for (kind, k), w in worst.items():
        print(f"emulation / bound  {kind:10s} {k:7s} {w:.3f}")


def test_mutations_are_rejected_on_the_emulation():
    seen = set()
    for B, G, T, D in CASES:
        for kind, beta in lr.GRID:
            for tag, c, kw in variants(B, G, T, D, beta):
                if tag == "ragged":
                    continue
                got = {k: t(v) for k, v in lr.emulate_masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, **kw).items()}
                ref = lr.masked_loss(c["preds"], c["targets"], c["tgt"], B, G, T, D, kind, beta, **kw)
                for label, k, m in lr.mutations(got, c, B, G, T, D, kind, beta, **kw):
                    assert nr.rejected(m, *ref[k]), f"{kind} beta={beta} {B, G, T, D} {tag}: mutation '{label}' of {k} accepted"
                    seen.add((kind, label, k))
    # every mutation of the list was made somewhere (beta = 1 makes the beta / delta ones no change: they come from 0.25 and 2)
    want = {("l1", "sign0", "dpreds"), ("l1", "factor2", "dpreds"), ("smooth_l1", "no_inv_beta", "loss"), ("smooth_l1", "no_inv_beta", "dpreds"),
            ("smooth_l1", "no_half", "loss"), ("smooth_l1", "no_half", "dpreds"), ("huber", "no_delta", "loss"), ("huber", "no_delta", "dpreds")}
    want |= {(k, "dpreds on a non-target row", "dpreds") for k in lr.KINDS}
    assert want <= seen, sorted(want - seen)


# ------------------------------------------------------------------------------------------------------------ C ABI
def loss_args(**kw):
    from wavjepa_amd import _abi
    a = _abi.STRUCTS["wj_loss_args"]()
    a.preds = a.targets = a.tgt = a.loss = a.workspace = 16          # never dereferenced: every call below is refused before a launch
    a.B, a.G, a.T, a.D = 2, 3, 5, 8
    a.gscale, a.beta = 1.0, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_of_the_loss_entry():
    from wavjepa_amd import _abi, ops
    lib = _abi.load()
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 == lib.wj_abi_version()
    assert [_abi.DEFINES[k] for k in ("WJ_LOSS_MSE", "WJ_LOSS_L1", "WJ_LOSS_SMOOTH_L1", "WJ_LOSS_HUBER")] == [0, 1, 2, 3]
    assert "wj_masked_loss" in _abi.FUNCTIONS and hasattr(lib, "wj_masked_loss")
    assert lib.wj_struct_size(b"wj_loss_args") == ctypes.sizeof(_abi.STRUCTS["wj_loss_args"])
    mse, loss = [n for n, _ in _abi._STRUCT_FIELDS["wj_mse_args"]], [n for n, _ in _abi._STRUCT_FIELDS["wj_loss_args"]]
    assert loss == mse + ["kind", "beta"]
    assert ops.workspace_bytes("wj_masked_loss", B=3, G=4, T=50) == ops.workspace_bytes("wj_masked_mse", B=3, G=4, T=50) == (2 + 600) * 4


def test_loss_entry_rejects_bad_arguments_without_a_gpu():
    """validation precedes every launch: each call here returns before one"""
    from wavjepa_amd import _abi, ops
    lib = _abi.load()
    call = lambda a: lib.wj_masked_loss(ctypes.byref(a), None)
    assert lib.wj_masked_loss(None, None) == -1
    for field in ("preds", "targets", "tgt", "loss", "workspace"):
        assert call(loss_args(**{field: None})) == -1, field
    assert call(loss_args(D=6)) == -1 and call(loss_args(T=0)) == -1 and call(loss_args(rows=16, n_rows=-1)) == -1
    for kind in (-1, 4, 17):
        assert call(loss_args(kind=kind)) == -3, kind
    for kind in (2, 3):
        for beta in (0.0, -1.0, math.nan, math.inf, -math.inf):
            assert call(loss_args(kind=kind, beta=beta)) == -1, (kind, beta)
    with pytest.raises(ValueError):
        ops.masked_loss(16, 16, 16, 16, 16, B=1, G=1, T=1, D=4, kind="hinge")


# ------------------------------------------------------------------------------------------------------------ module surface
def small_model(**kw):
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import JEPA
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    ext = ConvFeatureExtractor(conv_layers_spec=[(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)], in_channels=1)
    return JEPA(feature_extractor=ext, transformer_encoder_cfg=TransformerEncoderCFG.create(num_layers=1),
                transformer_encoder_layers_cfg=TransformerLayerCFG.create(d_model=128, nhead=2),
                transformer_decoder_cfg=TransformerEncoderCFG.create(num_layers=1),
                transformer_decoder_layers_cfg=TransformerLayerCFG.create(d_model=64, nhead=2), average_top_k_layers=1,
                process_audio_seconds=2.01, nr_samples_per_audio=2, **kw)


def test_loss_fn_maps_to_a_kernel_kind_or_raises():
    from wavjepa_amd.engine import EngineConfig
    from wavjepa_amd.jepa import loss_kind_of
    none = dict(reduction="none")
    assert loss_kind_of(None) == ("mse", 1.0) and loss_kind_of(nn.MSELoss(**none)) == ("mse", 1.0)
    assert loss_kind_of(nn.L1Loss(**none)) == ("l1", 1.0)
    assert loss_kind_of(nn.SmoothL1Loss(beta=0.25, **none)) == ("smooth_l1", 0.25) and loss_kind_of(nn.SmoothL1Loss(**none)) == ("smooth_l1", 1.0)
    assert loss_kind_of(nn.SmoothL1Loss(beta=0.0, **none)) == ("l1", 1.0)           # torch: beta = 0 is L1
    assert loss_kind_of(nn.HuberLoss(delta=2.0, **none)) == ("huber", 2.0)
    for bad in (nn.CosineSimilarity(), nn.BCELoss(**none), nn.Identity()):
        with pytest.raises(NotImplementedError):
            loss_kind_of(bad)
    for cls in (nn.MSELoss, nn.L1Loss, nn.SmoothL1Loss, nn.HuberLoss):
        for red in ("mean", "sum"):
            with pytest.raises(ValueError):
                loss_kind_of(cls(reduction=red))
    cfg = {f.name: f.default for f in EngineConfig.__dataclass_fields__.values()}
    assert cfg["loss_kind"] == "mse" and cfg["loss_beta"] == 1.0


def test_module_records_the_loss_only_when_it_is_not_mse():
    base = small_model()
    assert (base.loss_kind, base.loss_beta) == ("mse", 1.0) and "loss" not in base.hparams and "loss_beta" not in base.hparams
    m = small_model(loss_fn=nn.MSELoss(reduction="none"))
    assert m.loss_kind == "mse" and set(m.hparams) == set(base.hparams)
    m = small_model(loss_fn=nn.SmoothL1Loss(reduction="none", beta=0.5))
    assert (m.loss_kind, m.loss_beta) == ("smooth_l1", 0.5) and m.hparams["loss"] == "smooth_l1" and m.hparams["loss_beta"] == 0.5
    assert set(m.hparams) == set(base.hparams) | {"loss", "loss_beta"}
    m = small_model(loss_fn=nn.L1Loss(reduction="none"))
    assert m.hparams["loss"] == "l1"
    with pytest.raises(NotImplementedError):
        small_model(loss_fn=nn.CosineEmbeddingLoss())
    with pytest.raises(ValueError):
        small_model(loss_fn=nn.SmoothL1Loss())              # reduction='mean'
