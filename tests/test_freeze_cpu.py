"""Partial training on the host: the flat layout of a model frozen before it is laid out, JEPA.freeze / unfreeze, the unit table and the
backward's floor (wavjepa_amd/freeze.py), the option checks, the hyper-parameters, the launcher's keys and the optimiser's lr = 0
group.  The engine's launches are checked on the GPU (tests/test_freeze_gpu.py)."""
import os

import pytest
import torch

from tests import freeze_reference as FR
from tests.test_dropout_cpu import _jepa
from wavjepa_amd import freeze as F
from wavjepa_amd.params import FlatParams

L_ENC = L_DEC = 2            # of _jepa
SETS = dict(FR.SETS, B=["extract_audio.*", "feature_norms.*", "post_extraction_mapper.*", "encoder.layers.0.*"])     # (two student layers)


def student_names(m):
    return [n for n, _ in m.named_parameters() if F.is_student(n)]


def test_layout_of_a_model_frozen_before_construction_is_the_unfrozen_models():
    torch.manual_seed(5)
    plain, frozen = _jepa(), _jepa()
    assert frozen.freeze("extract_audio.*", "*.bias")
    a = FlatParams(plain, torch.device("cpu"), student=F.is_student)
    b = FlatParams(frozen, torch.device("cpu"), student=F.is_student)
    assert [(s.name, s.offset, s.numel, s.shape) for s in a.slots] == [(s.name, s.offset, s.numel, s.shape) for s in b.slots]
    assert a.n == b.n and a.tn == b.tn and a.enc_offset == b.enc_offset
    assert a.front_and_rest_ranges() == b.front_and_rest_ranges() and a.bucket_bounds(4) == b.bucket_bounds(4)
    # today's layout of a default model: the parameters with requires_grad, in named_parameters() order
    legacy = FlatParams(_jepa(), torch.device("cpu"))
    assert [(s.name, s.offset) for s in legacy.slots] == [(s.name, s.offset) for s in a.slots]
    for name in ("extract_audio.cnn.0.0.weight", "encoder.layers.0.linear1.bias"):
        assert b.ptr32(name) and b.gptr(name)                            # no KeyError
    assert not any(n.startswith(("teacher_encoder.", "pos_encoding_")) for n in b.by_name)
    # a frozen parameter exposes no gradient, a trainable one its view of the flat buffer
    params = dict(frozen.named_parameters())
    assert params["extract_audio.cnn.0.0.weight"].grad is None and params["encoder.layers.0.linear1.bias"].grad is None
    assert params["encoder.layers.0.linear1.weight"].grad.data_ptr() == b.gptr("encoder.layers.0.linear1.weight")


def test_freeze_unfreeze_and_pattern_errors():
    m = _jepa()
    names = student_names(m)
    got = m.freeze("extract_audio.*", "encoder.layers.[0-1].*")
    assert got == [n for n in names if n.startswith(("extract_audio.", "encoder.layers.0.", "encoder.layers.1."))] and got
    params = dict(m.named_parameters())
    assert all(not params[n].requires_grad for n in got)
    assert all(params[n].requires_grad for n in names if n not in got)
    assert m._frozen_names() == frozenset(got)
    back = m.unfreeze("encoder.layers.1.*")
    assert back == [n for n in names if n.startswith("encoder.layers.1.")] and all(params[n].requires_grad for n in back)
    assert m._frozen_names() == frozenset(got) - frozenset(back)
    params["mask_token"].requires_grad_(False)                         # by hand: honoured as well
    assert "mask_token" in m._frozen_names()
    biases = m.freeze("*.bias")
    assert biases == [n for n in names if n.endswith(".bias")]
    for bad in ("no_such_parameter.*", "teacher_encoder.*", "pos_encoding_encoder"):
        with pytest.raises(ValueError, match="matches no parameter"):
            m.freeze("extract_audio.*", bad)
        with pytest.raises(ValueError, match="matches no parameter"):
            m.unfreeze(bad)
    assert not any(p.requires_grad for n, p in m.named_parameters() if n.startswith("teacher_encoder."))


def plan_of(m, patterns, kept=None):
    names = student_names(m)
    frozen = FR.frozen_names(names, patterns)
    return F.BackwardPlan(F.skipped_units(names, frozen), L_ENC, L_DEC, kept), frozen, names


def test_unit_table_and_floor():
    m = _jepa()
    names = student_names(m)
    units = list(F.unit_table(names, ()))
    assert sorted(units) == sorted(F.chain(L_ENC, L_DEC)) and all(k == 0 and n > 0 for n, k in F.unit_table(names, ()).values())
    assert F.unit_table(names, ())["front"] == (4, 0)                   # feature_norms.* + post_extraction_mapper.*
    want = {
        "nothing": ([], "extract_audio", set()),
        "A": (SETS["A"], "front", {"extract_audio"}),
        "B": (SETS["B"], "encoder.layers.1", {"extract_audio", "front", "encoder.layers.0"}),
        "C": (SETS["C"], "extract_audio", {"decoder.layers.1"}),
        "D": (SETS["D"], "encoder_to_decoder_mapper", {"mask_token", "extract_audio", "front", "encoder.layers.0", "encoder.layers.1",
                                                       "encoder.norm"}),
        "everything": (["*"], None, set(F.chain(L_ENC, L_DEC))),
    }
    for key, (patterns, floor, skip) in want.items():
        plan, frozen, _ = plan_of(m, patterns)
        print(key, "floor", plan.floor, "skipped", sorted(plan.skip), "partly frozen", len(F.partly_frozen(names, frozen)), flush=True)
        assert plan.floor == floor and set(plan.skip) == skip, key
    # what the engine asks
    a = plan_of(m, SETS["A"])[0]
    assert a.reaches("front") and not a.reaches("extract_audio") and a.below("encoder.layers.0") and a.stack_walk("encoder", [0, 1]) == (True, None)
    b = plan_of(m, SETS["B"])[0]
    assert not b.reaches("front") and b.stack_walk("encoder", [0, 1]) == (True, 1) and b.stack_walk("decoder", [0, 1]) == (True, None)
    assert b.below("encoder_to_decoder_mapper") and not b.below("encoder.layers.1")
    d = plan_of(m, SETS["D"])[0]
    assert d.reaches("mask_token") and d.reaches("encoder_to_decoder_mapper") and not d.below("encoder_to_decoder_mapper")
    norm_only = plan_of(m, ["extract_audio.*", "feature_norms.*", "post_extraction_mapper.*", "encoder.layers.*"])[0]
    assert norm_only.floor == "encoder.norm" and norm_only.stack_walk("encoder", [0, 1]) == (False, None)
    none = plan_of(m, ["*"])[0]
    assert none.stack_walk("decoder", [0, 1]) == (False, None) and not none.reaches("decoder_to_encoder_mapper")
    # partly frozen units keep their launches: the frozen names are cleared afterwards
    c_frozen = plan_of(m, SETS["C"])[1]
    part = F.partly_frozen(names, c_frozen)
    assert part and all(n.endswith(".bias") and not n.startswith("decoder.layers.1.") for n in part)
    assert {F.section_of(n, L_ENC) for n in part} == {"dec", "enc:0", "enc:1", "front"}
    # LayerDrop: the floor is taken over the layers that run
    dropped = plan_of(m, SETS["A"] + ["feature_norms.*", "post_extraction_mapper.*"], kept=dict(enc=[1]))[0]
    assert dropped.floor == "encoder.layers.1" and dropped.stack_walk("encoder", [1]) == (True, 0)
    assert plan_of(m, SETS["A"] + ["feature_norms.*", "post_extraction_mapper.*"], kept=dict(enc=[]))[0].floor == "encoder.norm"


def test_feature_grad_mult_and_schedule_are_checked_and_recorded_only_when_set():
    off = _jepa()
    assert off.feature_grad_mult == 1.0 and off.freeze_feature_extractor_updates == 0 and off._frozen_names() == frozenset()
    assert not {"feature_grad_mult", "freeze_feature_extractor_updates", "freeze"} & set(off.hparams)
    for bad in (-0.1, 1.5, float("nan"), "half"):
        with pytest.raises(ValueError, match="feature_grad_mult"):
            _jepa(feature_grad_mult=bad)
    with pytest.raises(ValueError, match="freeze_feature_extractor_updates"):
        _jepa(freeze_feature_extractor_updates=-1)
    half = _jepa(feature_grad_mult=0.5)
    assert set(half.hparams) - set(off.hparams) == {"feature_grad_mult"} and half.hparams["feature_grad_mult"] == 0.5
    assert half._frozen_names() == frozenset()
    zero = _jepa(feature_grad_mult=0.0)
    conv = frozenset(n for n in student_names(zero) if n.startswith("extract_audio."))
    assert zero._frozen_names() == conv and conv                       # m = 0 is the frozen front-end
    held = _jepa(freeze_feature_extractor_updates=2)
    assert set(held.hparams) - set(off.hparams) == {"freeze_feature_extractor_updates"}
    seen = []
    for step in range(4):                                               # a function of global_step: a resumed run continues it
        held.global_step = step
        seen.append(held._frozen_names() == conv)
    assert seen == [True, True, False, False]


def test_launcher_reads_the_three_keys():
    import train
    from wavjepa_amd.config import load_config
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    off, _ = train.build_model(load_config(root, ["trainer.size=tiny"]))
    assert off._frozen_names() == frozenset() and not {"freeze", "feature_grad_mult", "freeze_feature_extractor_updates"} & set(off.hparams)
    on, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.freeze=[extract_audio.*]"]))
    assert set(on.hparams) - set(off.hparams) == {"freeze"} and tuple(on.hparams["freeze"]) == ("extract_audio.*",)
    assert on._frozen_names() == frozenset(n for n in student_names(on) if n.startswith("extract_audio."))
    two, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.freeze=['extract_audio.*', 'encoder.layers.[0-0].*']"]))
    assert any(n.startswith("encoder.layers.0.") for n in two._frozen_names()) and not any(n.startswith("encoder.layers.1.") for n in two._frozen_names())
    opts, _ = train.build_model(load_config(root, ["trainer.size=tiny", "trainer.feature_grad_mult=0.1", "trainer.freeze_feature_extractor_updates=500"]))
    assert opts.feature_grad_mult == 0.1 and opts.freeze_feature_extractor_updates == 500
    assert set(opts.hparams) - set(off.hparams) == {"feature_grad_mult", "freeze_feature_extractor_updates"}
    with pytest.raises(ValueError, match="matches no parameter"):
        train.build_model(load_config(root, ["trainer.size=tiny", "trainer.freeze=[no_such.*]"]))
    with pytest.raises(RuntimeError, match="feature_grad_mult"):
        train.build_model(load_config(root, ["trainer.size=tiny", "trainer.feature_grad_mult=2"]))


def test_lr_0_group_exists_only_while_something_is_frozen():
    from wavjepa_amd.jepa import FusedAdamW
    m = _jepa()
    opt = FusedAdamW(m, lr=1e-3)
    n_all = len(student_names(m))
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == n_all and "frozen" not in opt.param_groups[0]
    got = m.freeze("extract_audio.*")
    opt._sync_frozen_group()
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["frozen"] and opt.param_groups[1]["lr"] == 0.0 == opt.param_groups[1]["weight_decay"]
    assert len(opt.param_groups[1]["params"]) == len(got) and len(opt.param_groups[0]["params"]) == n_all - len(got)
    assert opt._frozen_assignment["extract_audio.cnn.0.0.weight"] == 1 and opt._frozen_assignment["mask_token"] == 0
    m.unfreeze("extract_audio.*")
    opt._sync_frozen_group()
    assert len(opt.param_groups) == 1 and len(opt.param_groups[0]["params"]) == n_all and opt._frozen_assignment is None
    # a model frozen before the optimiser exists, with groups of its own: the frozen group comes last, the others keep their settings
    m2 = _jepa(weight_decay_exclude="1d")
    m2.freeze("*.bias")
    opt2 = m2.configure_optimizers()["optimizer"]
    kinds = [(bool(q.get("frozen")), q["weight_decay"]) for q in opt2.param_groups]
    assert kinds[-1] == (True, 0.0) and [k[0] for k in kinds[:-1]] == [False] * (len(kinds) - 1) and len(kinds) == 3
    names = {id(p): n for n, p in m2.named_parameters()}
    assert all(names[id(p)].endswith(".bias") for p in opt2.param_groups[-1]["params"])
    assert not any(names[id(p)].endswith(".bias") for q in opt2.param_groups[:-1] for p in q["params"])
    sd = opt2.state_dict()
    assert len(sd["group_lr"]) == 2                                     # the frozen group follows the module, not the checkpoint
