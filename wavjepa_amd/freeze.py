"""Partial training: which parameters are frozen, which units of the step that leaves without parameter-gradient work, and where the
backward ends.  Pure arithmetic on parameter names (no torch, no GPU): the engine (encoder_engine.py, engine.py) asks it which
launches go out, JEPA.freeze / unfreeze which names a pattern selects.

A *unit* is the group of parameters one piece of the backward produces gradients for:
    mask_token | extract_audio | front (feature_norms.* + post_extraction_mapper.*) | encoder.layers.i | encoder.norm |
    encoder_to_decoder_mapper | decoder.layers.i | decoder.norm | decoder_to_encoder_mapper
A unit is *skipped* iff every parameter of it is frozen: none of its weight gradients, bias column sums or norm-parameter folds is
launched.  A partly frozen unit computes its gradients as always and the frozen ranges are cleared afterwards.

The *chain* orders the units by the way the gradient travels, loss last:
    extract_audio < front < encoder.layers.0 < ... < encoder.norm < encoder_to_decoder_mapper < mask_token < decoder.layers.0 < ...
    < decoder.norm < decoder_to_encoder_mapper
The *floor* is the lowest unit of the chain that is not skipped (and, under LayerDrop, runs in this step).  Nothing below it is
differentiated; the floor computes its own parameter gradients and no data gradient into its input.
"""
from __future__ import annotations

import fnmatch
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

NOT_STUDENT = ("teacher_encoder.", "pos_encoding_")      # the EMA copy and the fixed position tables: never trained, never laid out
FRONT_PREFIXES = ("feature_norms.", "post_extraction_mapper.")
_LAYER = re.compile(r"(encoder|decoder)\.layers\.(\d+)\.")


def is_student(name: str) -> bool:
    """True for the names FlatParams lays out for a JEPA module whether or not they are trainable."""
    return not name.startswith(NOT_STUDENT)


def unit_of(name: str) -> str:
    if name == "mask_token":
        return "mask_token"
    if name.startswith("extract_audio."):
        return "extract_audio"
    if name.startswith(FRONT_PREFIXES):
        return "front"
    m = _LAYER.match(name)
    if m:
        return f"{m.group(1)}.layers.{int(m.group(2))}"
    for unit in ("encoder.norm", "decoder.norm", "encoder_to_decoder_mapper", "decoder_to_encoder_mapper"):
        if name.startswith(unit + "."):
            return unit
    raise ValueError(f"parameter {name!r} belongs to no unit of the step")


def chain(l_enc: int, l_dec: int) -> List[str]:
    return (["extract_audio", "front"] + [f"encoder.layers.{i}" for i in range(l_enc)] + ["encoder.norm", "encoder_to_decoder_mapper",
            "mask_token"] + [f"decoder.layers.{i}" for i in range(l_dec)] + ["decoder.norm", "decoder_to_encoder_mapper"])


def match(names: Iterable[str], patterns: Sequence[str]) -> List[str]:
    """The student names that any of the fnmatch `patterns` selects, in the order of `names`.  A pattern that selects none: ValueError."""
    names = [n for n in names if is_student(n)]
    hit = set()
    for pat in patterns:
        if not isinstance(pat, str):
            raise ValueError(f"pattern {pat!r}: an fnmatch pattern on parameter names is expected")
        found = [n for n in names if fnmatch.fnmatchcase(n, pat)]
        if not found:
            raise ValueError(f"pattern {pat!r} matches no parameter of the student")
        hit.update(found)
    return [n for n in names if n in hit]


def unit_table(names: Iterable[str], frozen: Iterable[str]) -> Dict[str, Tuple[int, int]]:
    """unit -> (parameters, frozen parameters), units in order of first appearance"""
    frozen = set(frozen)
    out: Dict[str, Tuple[int, int]] = {}
    for n in names:
        u = unit_of(n)
        a, b = out.get(u, (0, 0))
        out[u] = (a + 1, b + int(n in frozen))
    return out


def skipped_units(names: Iterable[str], frozen: Iterable[str]) -> frozenset:
    return frozenset(u for u, (n, k) in unit_table(names, frozen).items() if k == n)


def partly_frozen(names: Iterable[str], frozen: Iterable[str]) -> List[str]:
    """The frozen names of units that are not skipped: their gradients are computed with the unit's and cleared afterwards."""
    names, frozen = list(names), set(frozen)
    skip = skipped_units(names, frozen)
    return [n for n in names if n in frozen and unit_of(n) not in skip]


def section_of(name: str, l_enc: int) -> str:
    """The backward's section tag (engine.backward: "dec", "enc:<i>", "front") behind which the gradient of `name` is final."""
    u = unit_of(name)
    if u.startswith("encoder.layers."):
        return "enc:" + u.rsplit(".", 1)[1]
    if u == "encoder.norm":
        return f"enc:{l_enc - 1}" if l_enc > 0 else "front"
    if u.startswith("decoder") or u == "encoder_to_decoder_mapper":
        return "dec"
    return "front"


class BackwardPlan:
    """Where one backward ends.  skip: the skipped units; kept: stack ("enc" / "dec") -> the layers that run in this step (LayerDrop;
    a stack that is not named runs every layer).  floor: the lowest unit of the chain that is neither skipped nor dropped, None when
    there is none (everything is frozen: the backward launches nothing)."""

    def __init__(self, skip: Iterable[str], l_enc: int, l_dec: int, kept: Optional[Dict[str, Sequence[int]]] = None):
        self.skip = frozenset(skip)
        self.chain = chain(l_enc, l_dec)
        self._index = {u: i for i, u in enumerate(self.chain)}
        dropped = set()
        for s, module, n in (("enc", "encoder", l_enc), ("dec", "decoder", l_dec)):
            if kept and kept.get(s) is not None:
                dropped |= {f"{module}.layers.{i}" for i in range(n)} - {f"{module}.layers.{int(i)}" for i in kept[s]}
        live = [i for i, u in enumerate(self.chain) if u not in self.skip and u not in dropped]
        self.level: Optional[int] = min(live) if live else None
        self.floor: Optional[str] = None if self.level is None else self.chain[self.level]

    def skipped(self, unit: str) -> bool:
        return unit in self.skip

    def reaches(self, unit: str) -> bool:
        """the backward gets as far down as `unit` (the floor is `unit` or lies below it)"""
        return self.level is not None and self.level <= self._index[unit]

    def below(self, unit: str) -> bool:
        """something trainable lies below `unit`: its data gradient is needed"""
        return self.level is not None and self.level < self._index[unit]

    def stack_walk(self, module: str, kept: Sequence[int]) -> Tuple[bool, Optional[int]]:
        """How far the backward of a stack goes -> (run the layers at all, stop): `kept` are the layers of the stack that ran, ascending.
        stop = None: down to the stack's input (something trainable lies below the stack); stop = j: the j-th kept layer is the floor --
        its own parameter gradients, no data gradient into its input.  (False, None): the floor is the stack's final norm or lies
        above the stack."""
        if self.level is None:
            return False, None
        first = self._index[f"{module}.layers.0"] if f"{module}.layers.0" in self._index else self._index[f"{module}.norm"]
        if self.level < first:
            return True, None
        if self.level >= self._index[f"{module}.norm"]:
            return False, None
        i = self.level - first
        return True, list(kept).index(i)


def check_grad_mult(m) -> float:
    """feature_grad_mult: the factor on the gradient that enters the conv stack (fairseq's GradMultiply), in [0, 1]"""
    try:
        v = float(m)
    except (TypeError, ValueError):
        raise ValueError(f"feature_grad_mult={m!r}: a number in [0, 1]") from None
    if not 0.0 <= v <= 1.0:
        raise ValueError(f"feature_grad_mult={m!r} must lie in [0, 1]")
    return v
