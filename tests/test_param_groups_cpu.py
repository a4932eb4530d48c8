"""Parameter groups of FusedAdamW, host side: wavjepa_amd.optim.param_groups on host-built models, the refused inputs, the group map
against a brute-force one, the default model's unchanged surface, the state_dict round trip, LambdaLR over groups, the launcher, the
C ABI of libwavjepa_hip_optim.so, and the mutations the bound must reject (tests/param_groups_reference.py).  None of this needs a GPU
(tests/test_param_groups_ops_gpu.py and tests/test_param_groups_gpu.py run the kernel and the step)."""
from __future__ import annotations

import ctypes
import functools
import inspect
import os

import numpy as np
import pytest
import torch

from tests import optimizer_reference as orf
from tests import param_groups_reference as pgr
from tests.norm_reference import f32eps, worst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRONT = ("extract_audio.", "feature_norms.", "post_extraction_mapper.")


def cfg(*over):
    from wavjepa_amd.config import load_config
    return load_config(os.path.join(ROOT, "configs"), list(over))


@functools.lru_cache(maxsize=None)
def model(size: str, *over):
    """a host-built model of the launcher's (never moved to a device)"""
    import train
    return train.build_model(cfg(f"trainer.size={size}", *over))[0]


def names_of(m):
    return [n for n, p in m.named_parameters() if p.requires_grad]


# ------------------------------------------------------------------------------------------------------------ param_groups
@pytest.mark.parametrize("size", ["tiny", "base", "large"])
def test_param_groups_on_host_built_models(size):
    from wavjepa_amd.optim import MAX_GROUPS, layer_id, param_groups
    m = model(size)
    params = dict(m.named_parameters())
    names = names_of(m)
    L = m.encoder.num_layers
    lr, wd = float(m.hparams["lr"]), float(m.hparams["adam_weight_decay"])
    # neither option: one group of everything, in the flat order
    one = param_groups(m)
    assert len(one) == 1 and one[0]["params"] == names and one[0]["lr"] == lr and one[0]["weight_decay"] == wd
    # "1d": exactly the parameters with ndim <= 1 plus the mask token, at weight decay 0
    two = param_groups(m, weight_decay_exclude="1d")
    assert len(two) == 2 and [g["weight_decay"] for g in two] == [wd, 0.0] and all(g["lr"] == lr for g in two)
    want = {n for n in names if params[n].ndim <= 1 or n == "mask_token"}
    assert set(two[1]["params"]) == want and "mask_token" in want and params["mask_token"].ndim == 3
    assert sorted(two[0]["params"] + two[1]["params"]) == sorted(names)
    assert all(n.endswith(("weight", "in_proj_weight")) and params[n].ndim >= 2 for n in two[0]["params"])
    # patterns on names
    pat = param_groups(m, weight_decay_exclude=["*.bias", "*norm*", "mask_token"], lr=1.0, weight_decay=0.5)
    assert pat[0]["weight_decay"] == 0.5 and pat[1]["weight_decay"] == 0.0 and pat[0]["lr"] == 1.0
    assert all(n.endswith(".bias") or "norm" in n or n == "mask_token" for n in pat[1]["params"]) and "mask_token" in pat[1]["params"]
    assert not [n for n in pat[0]["params"] if n.endswith(".bias") or "norm" in n]
    # layer-wise lr decay: BEiT's ids and scales, formed in double
    d = 0.75
    both = param_groups(m, weight_decay_exclude="1d", layer_lr_decay=d)
    assert len(both) == 2 * (L + 2) <= MAX_GROUPS
    if size == "large":
        assert L == 24 and len(both) == 52
    seen = []
    for g in both:
        ids = {layer_id(n, L) for n in g["params"]}
        assert len(ids) == 1
        i = ids.pop()
        assert g["lr"] == lr * d ** (L + 1 - i), (i, g["lr"])
        assert g["weight_decay"] in (0.0, wd) and all((n in want) == (g["weight_decay"] == 0.0) for n in g["params"])
        for n in g["params"]:
            if n.startswith(FRONT):
                assert i == 0, n
            elif n.startswith("encoder.layers."):
                assert i == int(n.split(".")[2]) + 1, n
            else:
                assert i == L + 1 and n.startswith(("encoder.norm.", "decoder.", "mask_token", "decoder_to_encoder_mapper.", "encoder_to_decoder_mapper.")), n
        seen += g["params"]
    assert sorted(seen) == sorted(names) and len(seen) == len(set(seen))          # every trainable parameter in exactly one group
    assert both[-1]["lr"] == lr and both[0]["lr"] == lr * d ** (L + 1)
    only = param_groups(m, layer_lr_decay=d)
    assert len(only) == L + 2 and all(g["weight_decay"] == wd for g in only)
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError):
            param_groups(m, layer_lr_decay=bad)
    with pytest.raises(ValueError):
        param_groups(m, weight_decay_exclude="2d")


def test_refused_groups():
    from wavjepa_amd.jepa import FusedAdamW
    from wavjepa_amd.optim import param_groups
    m = model("tiny")
    names = names_of(m)
    opt = lambda groups, **kw: FusedAdamW(m, lr=1e-3, weight_decay=0.04, groups=groups, **kw)
    good = param_groups(m, weight_decay_exclude="1d")
    assert len(opt(good).param_groups) == 2
    twice = [dict(g) for g in good]
    twice[1] = dict(twice[1], params=twice[1]["params"] + [twice[0]["params"][3]])
    with pytest.raises(ValueError, match=twice[0]["params"][3].replace(".", r"\.")):
        opt(twice)
    missing = [dict(good[0], params=good[0]["params"][:-1]), good[1]]
    with pytest.raises(ValueError, match=good[0]["params"][-1].replace(".", r"\.")):
        opt(missing)
    with pytest.raises(ValueError, match="64"):
        opt([{"params": [n]} for n in names[:64]] + [{"params": names[64:]}])
    assert len(opt([{"params": [n]} for n in names[:63]] + [{"params": names[63:]}]).param_groups) == 64
    with pytest.raises(ValueError, match="no_such"):
        opt([{"params": names + ["no_such.weight"]}])
    with pytest.raises(ValueError, match="betas"):
        opt([dict(good[0], betas=(0.8, 0.9)), good[1]])
    with pytest.raises(ValueError, match="eps"):
        opt([dict(good[0], eps=1e-3), good[1]])
    assert len(opt([dict(good[0], betas=(0.9, 0.98), eps=1e-6), good[1]]).param_groups) == 2       # the optimiser's own: accepted
    with pytest.raises(ValueError):
        opt([])
    # Parameters instead of names; lr / weight_decay default to the constructor's
    params = dict(m.named_parameters())
    o = opt([{"params": [params[n] for n in good[0]["params"]]}, {"params": good[1]["params"], "weight_decay": 0.0, "lr": 5e-4}])
    assert [(g["lr"], g["weight_decay"]) for g in o.param_groups] == [(1e-3, 0.04), (5e-4, 0.0)]
    assert [id(p) for p in o.param_groups[0]["params"]] == [id(params[n]) for n in good[0]["params"]]


def test_a_denoiser_takes_groups_and_keeps_its_default():
    """FusedAdamW(module, groups=...) is generic: the Denoiser stage is not refused; its own configure_optimizers builds the one group."""
    from wavjepa_amd.denoiser import Denoiser
    from wavjepa_amd.extractors import ConvFeatureExtractor
    from wavjepa_amd.jepa import FusedAdamW
    from wavjepa_amd.optim import layer_id, param_groups
    from wavjepa_amd.types import TransformerEncoderCFG, TransformerLayerCFG
    den = Denoiser(ConvFeatureExtractor(conv_layers_spec=[(32, 10, 5)] + [(32, 3, 2)] * 4 + [(32, 2, 2)], in_channels=1),
                   TransformerLayerCFG.create(d_model=64, nhead=2), TransformerEncoderCFG.create(num_layers=2), adam_weight_decay=0.04)
    names = names_of(den)
    params = dict(den.named_parameters())
    default = den.configure_optimizers()["optimizer"]
    assert len(default.param_groups) == 1 and default._assignment is None
    assert [id(p) for p in default.param_groups[0]["params"]] == [id(params[n]) for n in names]
    groups = param_groups(den, weight_decay_exclude="1d", layer_lr_decay=0.5)
    opt = FusedAdamW(den, lr=den.hparams["lr"], weight_decay=den.hparams["adam_weight_decay"], groups=groups)
    L = den.encoder.num_layers
    assert len(opt.param_groups) == len(groups) and 2 <= len(groups) <= 2 * (L + 2)
    assert sorted(n for g in opt.param_groups for n in g["names"]) == sorted(names) and set(opt._assignment) == set(names)
    for g in opt.param_groups:
        assert g["weight_decay"] == (0.0 if all(params[n].ndim <= 1 for n in g["names"]) else 0.04)
        assert all((params[n].ndim <= 1) == (g["weight_decay"] == 0.0) for n in g["names"])
    assert {g["lr"] for g in opt.param_groups} == {den.hparams["lr"] * 0.5 ** (L + 1 - i) for i in range(L + 2)
                                                  if any(layer_id(n, L) == i for n in names)}
    assert set(opt.state_dict()) == {"step", "lr", "m", "v", "group_lr", "group_weight_decay"}


# ------------------------------------------------------------------------------------------------------------ the map
class Odd(torch.nn.Module):
    """parameters whose sizes are no multiple of the granule: every slot but one ends in padding"""
    def __init__(self):
        super().__init__()
        self.extract_audio = torch.nn.Linear(5, 3)              # 15 + 3
        self.encoder = torch.nn.Linear(3, 7)                    # 21 + 7
        self.decoder = torch.nn.Linear(8, 2)                    # 16 + 2
        self.mask_token = torch.nn.Parameter(torch.zeros(1, 1, 9))


@pytest.mark.parametrize("size", ["tiny", "base", "odd"])
def test_group_map_equals_brute_force(size):
    from wavjepa_amd.optim import param_groups, resolve_groups
    from wavjepa_amd.params import ALIGN, FlatParams
    if size == "odd":
        m = Odd()
        groups = [{"params": [n]} for n in names_of(m)[:3]] + [{"params": names_of(m)[3:]}]
    else:
        m = model.__wrapped__(size)                                               # a model of its own: FlatParams re-points the parameters
        groups = param_groups(m, weight_decay_exclude="1d", layer_lr_decay=0.75)
    _, assignment = resolve_groups(m, groups, dict(lr=1e-3, weight_decay=0.04, betas=(0.9, 0.98), eps=1e-6))
    flat = FlatParams(m, torch.device("cpu"))
    assert ALIGN == pgr.GRANULE and flat.n % ALIGN == 0
    got = flat.group_map(assignment)
    assert got.dtype == torch.uint8 and got.shape == (flat.n // ALIGN,)
    elem = pgr.element_groups(flat.slots, assignment, flat.n)
    assert torch.equal(got, pgr.granule_map(elem))
    pads = [s for s in flat.slots if s.numel % ALIGN]
    assert bool(pads) == (size == "odd")                                          # (the launcher's models have none: Odd is here for them)
    for s in pads:                                                                # a slot's padding granule is its own
        assert int(got[(s.offset + s.numel) // ALIGN]) == assignment[s.name]
    assert len(set(got.tolist())) == len(groups)
    front, rest = flat.front_and_rest_ranges()
    assert front and rest
    for lo, hi in front + rest:                                                   # what a launch on [lo, hi) reads: map[lo / 8 + i / 8]
        assert lo % ALIGN == 0 and (hi - lo) % ALIGN == 0
        assert torch.equal(got[lo // ALIGN:hi // ALIGN].long().repeat_interleave(ALIGN), elem[lo:hi])
    with pytest.raises(ValueError, match=flat.slots[5].name.replace(".", r"\.")):
        flat.group_map({k: v for k, v in assignment.items() if k != flat.slots[5].name})


# ------------------------------------------------------------------------------------------------------------ default / grouped model
def test_default_model_is_what_it_was():
    from tests.test_recompute_cpu import DEFAULT_HPARAMS, plain_path
    from wavjepa_amd.jepa import JEPA, FusedAdamW
    m = model("tiny")
    assert m.weight_decay_exclude is None and m.layer_lr_decay == 1.0
    if plain_path():
        assert set(m.hparams) == DEFAULT_HPARAMS
    assert not {"weight_decay_exclude", "layer_lr_decay"} & set(m.hparams)
    sig = inspect.signature(JEPA.__init__).parameters                             # keywords through **kwargs: the named parameters are the reference's
    assert "weight_decay_exclude" not in sig and "layer_lr_decay" not in sig and sig["kwargs"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(FusedAdamW.__init__).parameters["groups"].default is None
    opt = m.configure_optimizers()["optimizer"]
    assert len(opt.param_groups) == 1 and opt._assignment is None
    want = [p for p in m.parameters() if p.requires_grad]
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in want]
    assert set(opt.param_groups[0]) >= {"params", "lr", "betas", "eps", "weight_decay"} and "names" not in opt.param_groups[0]
    sd_opt = FusedAdamW(m, lr=1e-3)
    object.__setattr__(sd_opt, "_module", type("M", (), {"_flat": None, "_engine": None})())
    assert set(sd_opt.state_dict()) == {"step", "lr", "m", "v"}


def test_grouped_model_hparams_and_state_round_trip():
    from wavjepa_amd.jepa import FusedAdamW
    m = model("tiny", "+optimizer.weight_decay_exclude=1d", "+optimizer.layer_lr_decay=0.75")
    assert m.hparams["weight_decay_exclude"] == "1d" and m.hparams["layer_lr_decay"] == 0.75
    assert set(m.hparams) - set(model("tiny").hparams) == {"weight_decay_exclude", "layer_lr_decay"}
    only = model("tiny", "+optimizer.weight_decay_exclude=['*.bias']")
    assert only.hparams["weight_decay_exclude"] == ("*.bias",) and "layer_lr_decay" not in only.hparams
    opt = m.configure_optimizers()["optimizer"]
    L = m.encoder.num_layers
    assert len(opt.param_groups) == 2 * (L + 2) and opt._assignment is not None
    stub = type("M", (), {"_flat": None, "_engine": None})()
    real = opt._module
    opt._module = stub
    for k, g in enumerate(opt.param_groups):
        g["lr"], g["weight_decay"] = 1e-4 * (k + 1), 0.01 * k
    sd = opt.state_dict()
    assert set(sd) == {"step", "lr", "m", "v", "group_lr", "group_weight_decay"}
    assert sd["group_lr"] == [1e-4 * (k + 1) for k in range(len(opt.param_groups))] and sd["lr"] == sd["group_lr"][0]
    opt._module = real
    fresh = m.configure_optimizers()["optimizer"]

    class Flat:                      # (load_state_dict touches the engine for the moments: none on this host)
        adam_m = adam_v = None
        def ensure_adam_state(self): pass
    eng = type("E", (), {"wait_optimizer": lambda self: None})()
    fresh._module = type("M", (), {"_flat": Flat(), "_engine": eng, "_ensure_engine": lambda self: eng})()
    fresh.load_state_dict(dict(sd, step=7))
    assert fresh._t == 7
    assert [g["lr"] for g in fresh.param_groups] == sd["group_lr"] and [g["weight_decay"] for g in fresh.param_groups] == sd["group_weight_decay"]
    with pytest.raises(ValueError):
        fresh.load_state_dict(dict(sd, group_lr=sd["group_lr"][:-1]))


def test_lambda_lr_scales_every_groups_initial_lr():
    from wavjepa_amd.jepa import FusedAdamW, cosine_schedule_with_warmup
    m = model("tiny")
    names = names_of(m)
    groups = [{"params": names[:5], "lr": 1e-3, "weight_decay": 0.4}, {"params": names[5:9], "lr": 1e-5, "weight_decay": 0.0},
              {"params": names[9:]}]
    opt = FusedAdamW(m, lr=3e-4, weight_decay=0.04, groups=groups)
    sched = cosine_schedule_with_warmup(opt, num_warmup_steps=2, num_training_steps=10)
    init = [1e-3, 1e-5, 3e-4]
    assert [g["initial_lr"] for g in opt.param_groups] == init and [g["lr"] for g in opt.param_groups] == [0.0, 0.0, 0.0]
    import math
    for step in range(1, 6):
        opt._t += 1                      # (LambdaLR warns when the optimiser has not stepped; the update needs a GPU)
        opt._opt_called = True
        sched.step()
        f = step / 2 if step < 2 else max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((step - 2) / 8))))
        assert [g["lr"] for g in opt.param_groups] == [x * f for x in init], step
        assert [g["weight_decay"] for g in opt.param_groups] == [0.4, 0.0, 0.04]


def test_launcher_reads_the_two_keys():
    import train
    assert train.optimizer_group_settings(cfg()) == {}
    assert train.optimizer_group_settings(cfg("+optimizer.weight_decay_exclude=1d")) == {"weight_decay_exclude": "1d"}
    assert train.optimizer_group_settings(cfg("+optimizer.layer_lr_decay=0.65")) == {"layer_lr_decay": 0.65}
    assert train.optimizer_group_settings(cfg("+optimizer.layer_lr_decay=1.0")) == {}
    assert train.optimizer_group_settings(cfg("+optimizer.weight_decay_exclude=['*.bias','mask_token']", "+optimizer.layer_lr_decay=0.9")) == \
        {"weight_decay_exclude": ("*.bias", "mask_token"), "layer_lr_decay": 0.9}
    # (the committed configs do not carry the keys, so the first line above is the .get(...) default at work)
    for name in os.listdir(os.path.join(ROOT, "configs", "optimizer")):           # the committed configs do not carry the keys
        text = open(os.path.join(ROOT, "configs", "optimizer", name)).read()
        assert "weight_decay_exclude" not in text and "layer_lr_decay" not in text


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_abi_of_the_optim_entry():
    """The entry lives in a library and a header of its own: what libwavjepa_hip.so exports and declares has not moved."""
    import subprocess
    from wavjepa_amd import _abi, ops
    rel, lib = _abi.load(), _abi.load("optim")
    assert _abi.DEFINES["WJ_ABI_VERSION"] == 17 == rel.wj_abi_version()
    assert "wj_adamw_groups_step" not in _abi.FUNCTIONS and "wj_adamw_groups_step" not in _abi.ENTRY_ARGS and not hasattr(rel, "wj_adamw_groups_step")
    assert _abi.LIBRARIES["optim"].entry_args == {"wj_adamw_groups_step": "wj_adamw_groups_args"}
    S = _abi.LIBRARIES["optim"].struct_types["wj_adamw_groups_args"]
    assert ctypes.sizeof(S) == 6 * 8 + 8 + 7 * 4 + 3 * 4 + 2 * 64 * 4 + 8 + 8 == lib.wj_optim_struct_size(b"wj_adamw_groups_args")
    old = [n for n, _ in _abi.STRUCTS["wj_adamw_args"]._fields_]
    new = [n for n, _ in S._fields_]
    assert new == [n for n in old if n not in ("lr", "weight_decay")] + ["n_groups", "lr", "weight_decay", "group_map", "first"]
    assert lib.wj_optim_struct_size(b"wj_adamw_args") == -1 and lib.wj_optim_struct_size(None) == -1
    out = subprocess.run(["nm", "-D", "--defined-only", _abi.LIBRARIES["optim"].path], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert exported == set(_abi.LIBRARIES["optim"].functions) == {"wj_adamw_groups_step", "wj_optim_struct_size", "wj_optim_workspace_bytes"}
    assert ops.ADAMW_MAX_GROUPS == 64 and ops.ADAMW_GRANULE == 8 and ops._ENTRY_STRUCT["wj_adamw_groups_step"] is S
    assert int(lib.wj_optim_workspace_bytes(b"wj_adamw_groups_step", ctypes.byref(S()))) == 0
    assert int(lib.wj_optim_workspace_bytes(b"wj_adamw_step", ctypes.byref(S()))) == -1
    assert int(lib.wj_optim_workspace_bytes(None, None)) == -1


def test_optim_entry_rejects_bad_arguments_without_a_gpu():
    from wavjepa_amd import _abi, ops
    lib = _abi.load("optim")
    S = _abi.LIBRARIES["optim"].struct_types["wj_adamw_groups_args"]
    ptr = 4096                                                  # never dereferenced: every call below is refused on the host
    good = dict(p=ptr, g=ptr, m=ptr, v=ptr, p_bf16=ptr, sumsq=ptr, n=1032, beta1=0.9, beta2=0.98, eps=1e-6, bc1=0.1, bc2=0.02, max_norm=5.0,
                grad_scale=1.0, n_groups=2, group_map=ptr, first=8)
    call = lambda **kw: int(lib.wj_adamw_groups_step(ctypes.byref(S(**dict(good, **kw))), None))
    assert int(lib.wj_adamw_groups_step(None, None)) == -1
    for name in ("p", "g", "m", "v", "group_map"):
        assert call(**{name: 0}) == -1, name
    for n in (0, -8, 4, 12, 1028, 1031, 1036):
        assert call(n=n) == -1, n                               # n % 8
    for first in (-8, 1, 4, 12, 1028):
        assert call(first=first) == -1, first                   # the first element off a granule
    for k in (0, -1, 65, 1000):
        assert call(n_groups=k) == -1, k
    assert call(p=ptr + 8) == -1 and call(g=ptr + 4) == -1 and call(m=ptr + 8) == -1 and call(v=ptr + 12) == -1 and call(p_bf16=ptr + 4) == -1
    with pytest.raises(_abi.WavJepaHipError):
        ops.adamw_groups_step(ptr, ptr, ptr, ptr, 12, lr=[1e-3], weight_decay=[0.0], group_map=ptr, first=0, beta1=0.9, beta2=0.98, eps=1e-6,
                              step=1, stream=0)
    with pytest.raises(ValueError):
        ops.adamw_groups_step(ptr, ptr, ptr, ptr, 8, lr=[1e-3] * 65, weight_decay=[0.0] * 65, group_map=ptr, first=0, beta1=0.9, beta2=0.98,
                              eps=1e-6, step=1, stream=0)


# ------------------------------------------------------------------------------------------------------------ mutations
N_MUT, LO_MUT = 1032, 8 * 129


@pytest.mark.parametrize("kind", ["randn", "clipped", "scaled", "mixed"])
@pytest.mark.parametrize("state", orf.STATES)
def test_every_mutation_is_claimed_and_the_emulation_is_inside(kind, state):
    """On the CPU, from the reference alone: each wrong lookup moves some element of p by more than twice its bound (so no output
    within the bound can hide it), while the fp32 emulation of the grouped step stays within the bound."""
    total = LO_MUT + N_MUT + 64
    for lay in ("alt2", "runs3", "all64", "absent"):
        gmap, n_groups = pgr.layout(lay, total // 8)
        emap = gmap.long().repeat_interleave(8)
        lr, wd = pgr.group_values(n_groups)
        c = orf.adamw_case(kind, state, N_MUT, "project", 300)
        Fc = pgr.common_fields(c["step"], c["grad_scale"])
        ss = orf.emulate_sumsq(c["g"])
        ss = torch.from_numpy(ss)
        elem = emap[LO_MUT:LO_MUT + N_MUT]
        ref = pgr.grouped_step(c["p"], c["g"], c["m"], c["v"], ss, Fc, lr, wd, elem)
        emu = pgr.emulate_grouped(c["p"], c["g"], c["m"], c["v"], ss, Fc, lr, wd, elem)
        for k in ("p", "m", "v", "p_bf16", "g"):
            assert worst(torch.from_numpy(emu[k]), *ref[k]) <= 1.0, (lay, k)
        got_p = torch.from_numpy(emu["p"])
        muts = pgr.mutations(c["p"], c["g"], c["m"], c["v"], ss, Fc, lr, wd, emap, LO_MUT, N_MUT, got_p, ref["p"][1],
                             pair=(0, 2) if lay == "absent" else (0, 1))
        assert [label for label, _, _ in muts] == list(pgr.MUTATIONS)
        for label, mut, claimed in muts:
            assert claimed, f"{lay} {kind} / {state}: mutation '{label}' is not separated by the reference"
            assert worst(mut, *ref["p"]) > 1.0, f"{lay} {kind} / {state}: mutation '{label}' accepted"
    # one group: the reference is optimizer_reference's own
    gmap, _ = pgr.layout("one", N_MUT // 8)
    c = orf.adamw_case(kind, state, N_MUT, "project", 300)
    ss = torch.from_numpy(orf.emulate_sumsq(c["g"]))
    H = c["H"]
    a = pgr.grouped_step(c["p"], c["g"], c["m"], c["v"], ss, pgr.common_fields(c["step"], c["grad_scale"]), [H["lr"]], [H["weight_decay"]],
                         gmap.long().repeat_interleave(8))
    b = orf.adamw_step(c["p"], c["g"], c["m"], c["v"], ss, orf.fields(H, c["step"], c["grad_scale"]))
    for k in a:
        assert torch.equal(a[k][0], b[k][0]) and torch.equal(a[k][1], b[k][1]), k
