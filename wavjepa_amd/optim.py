"""Parameter groups for FusedAdamW (wavjepa_amd.jepa): a learning rate and a weight decay per group, applied in ONE pass over the flat
parameter buffer (wj_adamw_groups_step, include/wavjepa_hip_optim.h).

`param_groups` builds the list FusedAdamW(module, groups=...) takes; `resolve_groups` is the validation FusedAdamW runs on any list.
A group is {"params": [parameter names or nn.Parameters], "lr": float, "weight_decay": float}; lr / weight_decay default to the
optimiser's.  Every trainable parameter belongs to exactly one group; betas and eps are the optimiser's own for all of them.
"""
from __future__ import annotations

import fnmatch
import re
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

from torch import nn

MAX_GROUPS = 64            # WJ_ADAMW_MAX_GROUPS of include/wavjepa_hip_optim.h (size="large" with both options below: 52)
FRONT_PREFIXES = ("extract_audio.", "feature_norms.", "post_extraction_mapper.")
_LAYER = re.compile(r"encoder\.layers\.(\d+)\.")


def trainable(module: nn.Module) -> List[Tuple[str, nn.Parameter]]:
    """the parameters the optimiser owns, in the order of the flat layout: for a module that lays out its whole student
    (JEPA.student_layout: freezing never moves a parameter) every student parameter, frozen or not; otherwise those with requires_grad"""
    if getattr(module, "student_layout", False):
        from .freeze import is_student
        return [(n, p) for n, p in module.named_parameters() if is_student(n)]
    return [(n, p) for n, p in module.named_parameters() if p.requires_grad]


def layer_id(name: str, num_layers: int) -> int:
    """BEiT's layer ids for layer-wise lr decay: 0 the conv front-end, its norm and its mapper; i + 1 the student's layer i;
    num_layers + 1 everything behind (encoder.norm, the two mappers, the predictor, the mask token)"""
    if name.startswith(FRONT_PREFIXES):
        return 0
    m = _LAYER.match(name)
    return int(m.group(1)) + 1 if m else num_layers + 1


def excluded_from_decay(name: str, p: nn.Parameter, rule: Union[None, str, Sequence[str]]) -> bool:
    """rule None: nothing; "1d": every parameter with ndim <= 1 (biases, norm scales) and the mask token -- timm's rule; otherwise a
    sequence of fnmatch patterns on the parameter's name"""
    if rule is None:
        return False
    if isinstance(rule, str):
        if rule != "1d":
            raise ValueError(f'weight_decay_exclude={rule!r}: None, "1d" or a sequence of fnmatch patterns on parameter names')
        return p.ndim <= 1 or name == "mask_token" or name.endswith(".mask_token")
    return any(fnmatch.fnmatchcase(name, pat) for pat in rule)


def param_groups(module: nn.Module, weight_decay_exclude: Union[None, str, Sequence[str]] = None, layer_lr_decay: float = 1.0,
                 lr: Optional[float] = None, weight_decay: Optional[float] = None) -> List[Dict[str, Any]]:
    """The groups of `module`'s trainable parameters, by name: parameters `weight_decay_exclude` selects get weight_decay 0, and with
    layer_lr_decay = d a parameter of layer id i (layer_id) gets lr * d ** (L + 1 - i), L the student's depth, formed in double.
    lr / weight_decay default to the module's hyper-parameters (lr, adam_weight_decay).  One group per (layer id, decayed or not) that
    holds a parameter, in that order; with neither option one group of everything."""
    hp = getattr(module, "hparams", {}) or {}
    lr = float(hp["lr"] if lr is None else lr)
    weight_decay = float(hp["adam_weight_decay"] if weight_decay is None else weight_decay)
    d = float(layer_lr_decay)
    if not 0.0 < d <= 1.0:
        raise ValueError(f"layer_lr_decay={layer_lr_decay!r} must lie in (0, 1]")
    L = 0
    if d != 1.0:
        enc = getattr(module, "encoder", None)
        if enc is None or not hasattr(enc, "num_layers"):
            raise ValueError("layer_lr_decay needs a module with an `encoder` stack (its layers carry the ids)")
        L = int(enc.num_layers)
    buckets: Dict[Tuple[int, bool], List[str]] = {}
    for name, p in trainable(module):
        key = (layer_id(name, L) if d != 1.0 else 0, excluded_from_decay(name, p, weight_decay_exclude))
        buckets.setdefault(key, []).append(name)
    groups = []
    for (i, no_decay), names in sorted(buckets.items()):
        groups.append({"params": names, "lr": lr * d ** (L + 1 - i) if d != 1.0 else lr, "weight_decay": 0.0 if no_decay else weight_decay})
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"{len(groups)} parameter groups: FusedAdamW takes at most {MAX_GROUPS}")
    return groups


def resolve_groups(module: nn.Module, groups: Sequence[Dict[str, Any]], defaults: Dict[str, Any]) -> Tuple[List[Dict[str, Any]], Dict[str, int]]:
    """FusedAdamW's view of a user's list: ([{"params": [Parameters], "names": [names], "lr", "weight_decay"}], {name: group index}).
    ValueError: more than MAX_GROUPS groups, a parameter in two groups or in none, a name or a Parameter the module does not train,
    a group that sets betas / eps other than the optimiser's."""
    groups = list(groups)
    if not groups:
        raise ValueError("groups is empty: pass None for the single default group")
    if len(groups) > MAX_GROUPS:
        raise ValueError(f"{len(groups)} parameter groups: FusedAdamW takes at most {MAX_GROUPS}")
    named = trainable(module)
    by_name = dict(named)
    name_of = {id(p): n for n, p in named}
    assignment: Dict[str, int] = {}
    out = []
    for k, grp in enumerate(groups):
        if not isinstance(grp, dict) or "params" not in grp:
            raise ValueError(f'group {k}: a dict with "params" (names or Parameters), "lr" and "weight_decay" is expected')
        unknown = set(grp) - {"params", "lr", "weight_decay", "betas", "eps"}
        if unknown:
            raise ValueError(f"group {k}: unknown keys {sorted(unknown)}")
        for key in ("betas", "eps"):
            if key in grp and (tuple(grp[key]) if key == "betas" else grp[key]) != (tuple(defaults[key]) if key == "betas" else defaults[key]):
                raise ValueError(f"group {k} sets {key}={grp[key]!r}: betas and eps are global in FusedAdamW ({key}={defaults[key]!r})")
        names = []
        for item in grp["params"]:
            name = item if isinstance(item, str) else name_of.get(id(item))
            if name is None or name not in by_name:
                raise ValueError(f"group {k}: {item if isinstance(item, str) else 'a Parameter'!r} is not a trainable parameter of the module")
            if name in assignment:
                raise ValueError(f"parameter {name!r} is in group {assignment[name]} and in group {k}: every parameter belongs to exactly one group")
            assignment[name] = k
            names.append(name)
        out.append({"params": [by_name[n] for n in names], "names": names, "lr": float(grp.get("lr", defaults["lr"])),
                    "weight_decay": float(grp.get("weight_decay", defaults["weight_decay"]))})
    for name, _ in named:
        if name not in assignment:
            raise ValueError(f"parameter {name!r} is in no group: every trainable parameter belongs to exactly one group")
    return out, assignment
